"""Long-lived objects: one scene rebuilt and refit across the build's regimes, one scene whose instances come and
go, one render target and camera sent through every trace kernel, three targets in flight across a refit.

The rest of the suite makes a fresh context, scene, camera and target for every call or two. The library is
written for the opposite: grow-only buffers, bound replicas that the last reader of one build zeroes for the
next, a per-tile cost table, a ray queue and a shadow plane that stay with the target. The walks are in
tests/long_lived_scenes.py; tests/test_oracle_long_lived.py asserts, without a GPU, that every step differs from
the one before it in what such state would carry over. Here every step is compared with the oracle: the export
bit for bit (keys, permutation, triangle records, reachable node records), frames and counters, the refits with
orc_bvh_refit and a rebuild's frame, the queries with the brute-force restatements of tests/test_gpu_rays.py,
tests/test_points_abi.py and tests/test_gpu_attrs.py, the ray queue's region counts with
test_gpu_ray_queue.survivor_bounds.

That the walks can fail was shown on scratch copies of the library, each with one store removed that changes
no address and no bound, loaded through BEAM_HIP_LIB, one GPU run per copy (nothing of it is committed):

(a1) no clear_replicas in the one-chunk branch of the chunk kernel (k_tree_chunk). New file: all three walks
     fail at step 1, the 3-triangle scene after 513 triangles: its first refit leaves the 4x-out box in the
     replicas and the second one's records differ from orc_bvh_refit's; test_instances_come_and_go fails too
     (the second build of its 126-triangle scene gets other keys). tests/test_gpu_build_sizes.py: 1 of 43
     fails (test_build_and_refit_at_regime_edges[2-2-0], the 2-triangle refit); tests/test_gpu_refit.py and
     tests/test_gpu_ray_queue.py pass.
(a2) no clear_replicas in k_chunk_table_lds. New file: the BVH4 walk fails at step 4 (131,073 triangles:
     23,227 records differ after the pair of refits), the BVH2 walk at step 1 (the 3-triangle build after 513
     triangles, whose last reader under BVH2 is this kernel: other keys); the leaf-1 walk, which stays below
     131,073 triangles, passes. tests/test_gpu_refit.py: 1 of 4 fails (test_refit_matches_oracle_and_rebuild
     for BVH2, at its third refit); tests/test_gpu_build_sizes.py and tests/test_gpu_ray_queue.py pass: no
     build of theirs follows a larger one on the same scene.
(b)  no shadow = 0 store for the rays k_cull culls. New file: test_one_target_through_every_kernel_kind fails
     on both streams at step 5, the compacted shadow frame of the wire after the dense scene's: 2,294 shadow
     bytes differ, exactly the culled-and-shadowed pixels tests/test_oracle_long_lived.py counts from the
     oracle. tests/test_gpu_ray_queue.py: 1 of 72 fails (test_fused_shadow, on what a fresh shadow plane
     happens to hold); tests/test_gpu_build_sizes.py and tests/test_gpu_refit.py pass.

The walks found no defect in the library: every step equals the oracle on the unedited build.

Measured on an MI355X: run alone the file takes 15.9 s of wall time (8 tests), 11.5 s of it PyTorch's start in
the first test that makes a query or a HIP stream, which the whole suite pays once elsewhere; the BVH4 walk takes
2.3 s with its CPU oracle builds (the 524,289-triangle step among them), the BVH2 walk 1.2 s, every other test
0.1 s or less.
"""
import numpy as np
import pytest

import long_lived_scenes as L
from raytracercuda_amd import beam, scenes
from test_gpu_build_sizes import compare
from test_gpu_ray_queue import SCENES, expected, layout, region_counts, survivor_bounds
from test_gpu_variants import check, expect

pytestmark = pytest.mark.gpu

ID = scenes.IDENTITY
MISS = np.uint32(0xFFFFFFFF)


def shoot(cam, rt, scene, eye):
    """A counting and a plain trace into the target, as test_gpu_variants.render: (frame, counters)."""
    cnt = cam.traceCounters(eye, ID, scene, rt)
    assert cam.trace(eye, ID, scene, rt) == 0
    return {k: v.reshape(-1) for k, v in rt.read().items()}, cnt


def oracle_shot(oracle, obvh, eye, window):
    err, rays = oracle.camera_rays(L.FRAME_W, L.FRAME_H, *window)
    assert err == 0
    packed, tri, t, cnt = obvh.render(rays, eye, ID, counters=True)
    return {"packed": packed, "tri_id": tri, "t": t}, cnt


# ---- 1. one scene across the build's regimes -----------------------------------------------------------------
def set_positions(keep, meshes):
    for m, d in zip(keep, meshes):
        assert m.setVertexData(d["pos"], d["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0


def expected_sort_path(step):
    if step.kind in ("skew", "equal"):
        return beam.SORT_MSD_SKEW  # test_build_skewed_top_digit, test_build_constant_digits
    return beam.SORT_MSD if step.n >= L.MSD_MIN_N else beam.SORT_LSD


@pytest.mark.parametrize("walk,width,leaf", [("full", 4, 4), ("full", 2, 4), ("short", 4, 1)],
                         ids=["bvh4", "bvh2", "leaf1"])
def test_one_scene_rebuilt_across_the_regimes(oracle, walk, width, leaf):
    steps = L.WALKS[walk][0]
    ctx = beam.Context(device=0, bvh_width=width, leaf_size=leaf)
    try:
        scene = beam.IScene.create(ctx)
        cam = beam.ICamera.create(ctx)
        assert cam.setInitialRays(L.FRAME_W, L.FRAME_H, *scenes.RAYS_SQUARE) == 0
        rt = beam.IRenderTarget.createOffscreen(ctx, L.FRAME_W, L.FRAME_H)
        keep = []
        for i, s in enumerate(steps):
            where = f"step {i} ({s.n} triangles, {L.regime(s.n)})"
            for m in keep:
                scene.removeMesh(m)
                m.destroy()
            meshes = L.step_meshes(walk, i)
            keep = beam.upload_meshes(ctx, scene, meshes)
            st = scene.updateGPUScene(stats=True)
            assert st["num_tris"] == s.n and st["bvh_width"] == width, where
            if s.n > L.CHUNK:
                assert st["sort_path"] == expected_sort_path(s), where
            obvh = oracle.bvh_build(list(meshes), leaf, width)
            try:
                compare(*scene.export(), obvh)
                eye, window = L.view(meshes)
                check(*shoot(cam, rt, scene, eye), *oracle_shot(oracle, obvh, eye, window))
                if s.refit:
                    set_positions(keep, L.moved(meshes, 4.0))
                    scene.refitGPUScene()
                    back = L.moved(meshes, 0.25)
                    set_positions(keep, back)
                    assert scene.refitGPUScene(stats=True)["num_tris"] == s.n
                    obvh.refit(list(back))
                    compare(*scene.export(), obvh)
                    # the frame equals a full rebuild's on the moved vertices; the counters are the refitted tree's
                    f, cnt = shoot(cam, rt, scene, eye)
                    rebuilt, _ = oracle_shot(oracle, oracle.bvh_build(list(back), leaf, width), eye, window)
                    _, rcnt = oracle_shot(oracle, obvh, eye, window)
                    check(f, cnt, rebuilt, rcnt)
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from e
    finally:
        ctx.close()


# ---- 2. instances and queries on the same scene ------------------------------------------------------------------
def test_instances_come_and_go(ctx, oracle):
    from test_gpu_attrs import assert_rows, records
    from test_gpu_attrs import expected as expected_rows
    from test_gpu_instances import pretransformed
    from test_gpu_points import assert_records, tri_vertices
    from test_gpu_rays import assert_hits, oracle_anyhit, oracle_closest
    from test_points_abi import brute_force

    scene = beam.IScene.create(ctx)
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(L.FRAME_W, L.FRAME_H, *scenes.RAYS_SQUARE) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, L.FRAME_W, L.FRAME_H)
    made = {}

    def imesh(m):
        if id(m) not in made:
            tmp = beam.IScene.create(ctx)
            made[id(m)] = beam.upload_meshes(ctx, tmp, [m])[0]
            tmp.destroy()
        return made[id(m)]

    def verify(entries, seed):
        pre = pretransformed(entries)
        ntri = sum(np.asarray(m["idx"]).size // 3 for m in pre)
        st = scene.updateGPUScene(stats=True)
        assert st["num_tris"] == ntri and st["num_meshes"] == len(entries)
        obvh = oracle.bvh_build(pre, 4, 4)
        compare(*scene.export(), obvh)
        check(*shoot(cam, rt, scene, L.INSTANCE_EYE), *oracle_shot(oracle, obvh, L.INSTANCE_EYE, scenes.RAYS_SQUARE))
        o, d, a, b, pts = L.query_batch(pre, seed)
        res = scene.traceRays(o, d, counters=True)
        occ = scene.traceRays(a, b - a, any_hit=True)["occluded"]
        if pre:
            exp, cnt = oracle_closest(oracle, obvh, pre, o, d, per=L.QUERY_N)
            hits = int((exp["tri_id"] != MISS).sum())
            assert 30 <= hits <= L.QUERY_N - 30, hits  # hits and misses both
            assert_hits(res, exp)
            assert list(map(int, res["counters"])) == list(map(int, cnt))
            eocc, _ = oracle_anyhit(obvh, a, b)
            assert 30 <= int(eocc.sum()) <= L.QUERY_N - 30
            assert np.array_equal(occ, eocc)
        else:
            assert np.all(res["tri_id"] == MISS) and np.all(np.isposinf(res["t"])) and not occ.any()
        assert_records(scene.closestPoints(pts), brute_force(pts, np.inf, tri_vertices(pre)), what=f"{len(entries)} entries")
        rec = records(res["t"], res["u"], res["v"], res["tri_id"])
        for r in ((beam.VERTEX_DATA_POSITION, 3, 0), (beam.ATTR_MESH_FACE, 2, 0)):
            got, = scene.hitAttributes(rec, [r])
            assert_rows(got, expected_rows(pre, rec, *r), f"request {r} with {len(entries)} entries")

    first, second, third = L.instance_walk()
    for k, (m, x) in enumerate(first):
        assert scene.addInstance(imesh(m), x) == k
    verify(first, 1)
    scene.removeInstance(0)
    assert scene.addInstance(imesh(second[-1][0]), second[-1][1]) == len(second) - 1
    verify(second, 2)
    for _ in second:
        scene.removeInstance(0)
    verify(third, 3)
    rt.destroy()
    cam.destroy()
    scene.destroy()


# ---- 3. one render target and one camera through every kernel kind ---------------------------------------------
def build_scenes(ctx):
    scs, keep = {}, {}
    for name in ("dense", "wire"):
        scs[name] = beam.IScene.create(ctx)
        keep[name] = beam.upload_meshes(ctx, scs[name], SCENES[name])
        scs[name].updateGPUScene()
    ctx.sync()  # the host copy of the scene boxes has arrived: the packet steps take packets
    return scs, keep


def run_sequence(ctx, oracle, frames, stream=None):
    scs, keep = build_scenes(ctx)
    cam = beam.ICamera.create(ctx)
    rts = {"big": beam.IRenderTarget.createOffscreen(ctx, L.W, L.H),
           "small": beam.IRenderTarget.createOffscreen(ctx, 64, 64)}
    if stream is not None:
        for rt in rts.values():
            rt.setStream(stream)
    rays = None
    for i, fr in enumerate(frames):
        where = f"step {i} ({fr.scene}, {fr.kind}, {fr.mode})"
        if (fr.w, fr.h, fr.window) != rays:
            assert cam.setInitialRays(fr.w, fr.h, *L.WINDOWS[fr.window]) == 0
            rays = (fr.w, fr.h, fr.window)
        ctx.set_param("trace_variant", fr.variant)
        ctx.set_param("trace_sched", fr.sched)
        ctx.set_param("cull_tiles", fr.tiles)
        rt, sc = rts[fr.target], scs[fr.scene]
        if fr.cost:
            rt.debugTileCosts(set=L.cost_table(fr.cost))
        assert ctx.lib.bm_rt_clear(rt.h, L.SENTINEL) == 0
        exp, ecnt = L.frame_planes(oracle, fr)
        cnt = None
        if fr.mode == "bands":
            assert cam.traceBands(fr.eye, ID, sc, rt, *L.BANDS) == 0
        elif fr.mode == "count":
            cnt = (cam.traceCounters(fr.eye, ID, sc, rt) if fr.light is None else
                   cam.traceShadowCounters(fr.eye, ID, sc, rt, fr.light))
        elif fr.light is None:
            assert cam.trace(fr.eye, ID, sc, rt) == 0
        else:
            assert cam.traceShadow(fr.eye, ID, sc, rt, fr.light) == 0
        assert rt.traceKind() == fr.kind, where
        counts = rt.rayQueueCounts() if fr.kind == "cull+quads" and fr.mode == "trace" else None
        f = rt.read()
        if fr.light is not None:
            f["shadow"] = rt.readShadow()
        try:
            if fr.mode == "bands":
                written = 0
                for local, rows in L.band_rows(fr.h, *L.BANDS):
                    k = rows.stop - rows.start
                    for plane, want in exp.items():
                        got = f[plane][local:local + k].view(np.uint32)
                        assert np.array_equal(got, want.reshape(fr.h, fr.w)[rows].view(np.uint32)), (plane, rows)
                    written = local + L.BANDS[0]
                assert np.all(f["packed"][written:] == L.SENTINEL), "rows past the rank's bands were written"
            else:
                check({k: v.reshape(-1) for k, v in f.items()}, cnt if cnt is not None else ecnt, exp, ecnt)
            if counts is not None:
                regions, tpr = layout(fr.w, fr.h, fr.tiles)
                assert counts.shape == (regions,)
                sure, maybe = survivor_bounds(oracle, fr.scene, fr.w, fr.h, eye=fr.eye, cam=L.WINDOWS[fr.window])
                lo, hi = region_counts(sure, tpr), region_counts(maybe, tpr)
                bad = np.nonzero((counts < lo) | (counts > hi))[0]
                assert bad.size == 0, f"region counts outside the oracle's bounds at regions {bad[:8]}"
        except AssertionError as e:
            raise AssertionError(f"{where}: {e}") from e
    for rt in rts.values():
        rt.destroy()
    cam.destroy()
    for sc in scs.values():
        sc.destroy()
    del keep


@pytest.mark.parametrize("own_stream", [False, True], ids=["context-stream", "own-stream"])
def test_one_target_through_every_kernel_kind(oracle, own_stream):
    st = None
    if own_stream:
        import torch
        st = torch.cuda.Stream()
    ctx = beam.Context(device=0)
    try:
        run_sequence(ctx, oracle, L.SEQUENCE, None if st is None else st.cuda_stream)
    finally:
        ctx.close()


def test_queued_shadows_on_one_target(oracle):
    ctx = beam.Context(device=0, shadow_queue=True)
    try:
        run_sequence(ctx, oracle, L.QUEUE_SEQUENCE)
    finally:
        ctx.close()


def test_three_targets_in_flight_across_a_refit(oracle):
    import torch

    ctx = beam.Context(device=0)
    try:
        scs, keep = build_scenes(ctx)
        cam = beam.ICamera.create(ctx)
        assert cam.setInitialRays(L.W, L.H, *scenes.RAYS_SQUARE) == 0
        streams = [torch.cuda.Stream() for _ in range(3)]
        rts = [beam.IRenderTarget.createOffscreen(ctx, L.W, L.H) for _ in streams]
        for rt, st in zip(rts, streams):
            rt.setStream(st.cuda_stream)
        moved = L.dense_moved()
        for k in range(1, L.FLIGHT_FRAMES + 1):
            name = L.flight_scene(k)
            for rt, eye in zip(rts, L.FLIGHT_EYES[name]):
                assert cam.trace(eye, ID, scs[name], rt) == 0
            if k == 6:  # the refit right behind the traces: those frames still see the old vertices
                set_positions(keep["dense"], moved)
                scs["dense"].refitGPUScene()
                for j, (rt, eye) in enumerate(zip(rts, L.FLIGHT_EYES["dense"])):
                    exp, ecnt = expected(oracle, "dense", L.W, L.H, eye=eye)
                    check({p: v.reshape(-1) for p, v in rt.read().items()}, ecnt, exp, ecnt)
        assert L.flight_scene(L.FLIGHT_FRAMES) == "dense"
        for rt, eye in zip(rts, L.FLIGHT_EYES["dense"]):
            exp, ecnt = expect(oracle, moved, L.W, L.H, scenes.RAYS_SQUARE, eye, ID)
            check({p: v.reshape(-1) for p, v in rt.read().items()}, ecnt, exp, ecnt)
        for rt in rts:
            rt.destroy()
    finally:
        ctx.close()
