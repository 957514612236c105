"""GPU parity of every ray kernel on rays whose traversal stacks leave LDS.

Every ray kernel keeps the first entries of a ray's stack in LDS (24 in the ray-quad and ray-query kernels,
8, 12 or 16 in the single-lane kernels) and the rest in a global overflow area laid out [depth - LDS][slot]
(reserve_overflow in bm_api.cpp; the wave-packet kernel shares one 96-entry LDS stack instead). The meshes
of the older parity tests never hold more than 12 entries (tests/test_oracle_deep_stack.py prints their
depths), so on them the overflow side never runs. The scenes of tests/deep_scenes.py need 30 to 63 entries
for a quarter to all of the rays of each frame and batch below; tests/test_oracle_deep_stack.py asserts
that, and that the oracle agrees with the exhaustive test on them, without a GPU.

All comparisons are bit for bit with the oracle (ids, packed colours, the bits of t, u and v, the shadow
bytes, the traversal counters). The oracle's answers are computed once per process (deep_scenes.expected,
query_expected) and shared.
"""
import numpy as np
import pytest

import deep_scenes as ds
from raytracercuda_amd import beam, scenes
from test_gpu_variants import COMPACT, PACKET, PRIO12, QUAD, vctx  # noqa: F401 (vctx: the fixture over VARIANTS)

pytestmark = pytest.mark.gpu

WIDTHS = [4, 2]  # BVH2: every variant hands the frame to the single-lane kernels (12 or 16 entries in LDS)
SCENE_IDS = [s[0] for s in ds.SCENES]
MAX_STACK8 = 160


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


def trace(ctx, scene, size, eye, orient, light=None, counters=True):
    """Frame (and counters: the counting kernels, then the plain ones into the same target)."""
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(*size, *ds.CAM) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, *size)
    cnt = None
    if light is None:
        if counters:
            cnt = cam.traceCounters(eye, orient, scene, rt)
        assert cam.trace(eye, orient, scene, rt) == 0
    else:
        if counters:
            cnt = cam.traceShadowCounters(eye, orient, scene, rt, light)
        assert cam.traceShadow(eye, orient, scene, rt, light) == 0
    f = {k: v.reshape(-1) for k, v in rt.read().items()}
    if light is not None:
        f["shadow"] = rt.readShadow().reshape(-1)
    rt.destroy()
    cam.destroy()
    return f, cnt


def check_frame(f, e, what=""):
    for k, want in e.frame.items():
        got = bits(f[k]) if f[k].dtype == np.float32 else f[k]
        want = bits(want) if want.dtype == np.float32 else want
        assert np.array_equal(got, want), f"{what} {k}: {int((got != want).sum())} of {want.size} pixels differ"


def deep_enough(e, width=4):
    """The fixture's own condition (asserted without a GPU in test_oracle_deep_stack.py for BVH4 and BVH2)."""
    assert e.stats[f">{ds.QUAD_LDS}"] >= 0.25 and e.stats["deepest"] <= (MAX_STACK8 if width == 8 else ds.MAX_STACK)


# ---- 1. every trace variant: frames and counters -------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", SCENE_IDS)
def test_variant_deep_frames_and_counters(vctx, oracle, name, width):
    _, dup, leaf = ds.scene_of(name)
    ctx = vctx(leaf_size=leaf, bvh_width=width)
    scene, keep = build(ctx, ds.deep_meshes(dup))
    for view in ds.VIEWS:
        for size in ds.SIZES:
            e = ds.expected(oracle, name, width, view, size)
            deep_enough(e, width)
            f, cnt = trace(ctx, scene, size, e.eye, e.orient)
            what = f"{name} BVH{width} {view} {size[0]}x{size[1]}"
            print(f"{what}: {ds.fmt(e.stats)}")
            check_frame(f, e, what)
            assert list(map(int, cnt)) == list(map(int, e.cnt)), what
    scene.destroy()


@pytest.mark.skipif(not beam.ab_build(), reason="BVH8 is built into A/B builds only (BM_TRACE_AB=1)")
@pytest.mark.parametrize("name", SCENE_IDS)
def test_bvh8_deep_frames_and_shadow_rays(oracle, name):
    _, dup, leaf = ds.scene_of(name)
    ctx = beam.Context(device=0, leaf_size=leaf, bvh_width=8)
    scene, keep = build(ctx, ds.deep_meshes(dup))
    for view in ds.VIEWS:
        for size in ds.SIZES:
            light = ds.LIGHT if size == ds.SIZES[0] else None
            e = ds.expected(oracle, name, 8, view, size, light=light)
            deep_enough(e, 8)
            f, cnt = trace(ctx, scene, size, e.eye, e.orient, light=light)
            what = f"{name} BVH8 {view} {size[0]}x{size[1]}"
            print(f"{what}: {ds.fmt(e.stats)}")
            check_frame(f, e, what)
            assert list(map(int, cnt)) == list(map(int, e.cnt)), what
    scene.destroy()
    ctx.close()


# ---- 2. shadow rays: fused and as a queue pass ---------------------------------------------------------
@pytest.mark.parametrize("queue", [False, True], ids=["fused", "queue"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", SCENE_IDS)
def test_variant_deep_shadow_rays(vctx, oracle, name, width, queue):
    _, dup, leaf = ds.scene_of(name)
    ctx = vctx(leaf_size=leaf, bvh_width=width, shadow_queue=queue)
    scene, keep = build(ctx, ds.deep_meshes(dup))
    size = ds.SIZES[0]
    for view in ds.VIEWS:
        e = ds.expected(oracle, name, width, view, size, light=ds.LIGHT)
        deep_enough(e, width)
        assert e.stats["shadow>24"] >= 0.25
        f, cnt = trace(ctx, scene, size, e.eye, e.orient, light=ds.LIGHT)
        what = f"{name} BVH{width} {view} shadow"
        print(f"{what}: {ds.fmt(e.stats)}")
        check_frame(f, e, what)
        assert list(map(int, cnt)) == list(map(int, e.cnt)), what
    scene.destroy()


# ---- 3. bands ------------------------------------------------------------------------------------------
def test_variant_deep_bands(vctx, oracle):
    ctx = vctx()
    scene, keep = build(ctx, ds.deep_meshes(0))
    (w, h), bh, n = ds.SIZES[0], 16, 3
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(w, h, *ds.CAM) == 0
    for view in ("axis", "mixed"):
        e = ds.expected(oracle, "deep", 4, view, (w, h))
        got = {k: np.zeros((h, w), v.dtype) for k, v in e.frame.items()}
        bands = (h + bh - 1) // bh
        for r in range(n):
            mine = [b for b in range(bands) if b % n == r]
            rt = beam.IRenderTarget.createOffscreen(ctx, w, len(mine) * bh)
            assert cam.traceBands(e.eye, e.orient, scene, rt, bh, n, r) == 0
            part = rt.read()
            for i, b in enumerate(mine):
                rows = slice(b * bh, min((b + 1) * bh, h))
                for k in got:
                    got[k][rows] = part[k][i * bh:i * bh + rows.stop - rows.start]
            rt.destroy()
        check_frame({k: v.reshape(-1) for k, v in got.items()}, e, f"bands {view}")
    cam.destroy()
    scene.destroy()


# ---- 4. small grids: a workgroup walks many tiles and reuses its overflow slots ------------------------
@pytest.mark.parametrize("variant", [None, PRIO12, QUAD, COMPACT], ids=["default", "single-lane", "quad", "compact"])
@pytest.mark.parametrize("grid", [1, 2])
def test_small_grids_reuse_their_slots(oracle, grid, variant):
    params = {"trace_grid": grid}
    if variant is not None:
        params["trace_variant"] = variant
    ctx = beam.Context(device=0, params=params)
    deep, keep = build(ctx, ds.deep_meshes(0))
    for view in ds.VIEWS:
        for size in ds.SIZES:
            e = ds.expected(oracle, "deep", 4, view, size)
            f, cnt = trace(ctx, deep, size, e.eye, e.orient)
            check_frame(f, e, f"grid {grid} {view} {size}")
            assert list(map(int, cnt)) == list(map(int, e.cnt))
    e = ds.expected(oracle, "deep", 4, "mixed", ds.SIZES[0], light=ds.LIGHT)
    f, cnt = trace(ctx, deep, ds.SIZES[0], e.eye, e.orient, light=ds.LIGHT)
    check_frame(f, e, f"grid {grid} shadow")
    assert list(map(int, cnt)) == list(map(int, e.cnt))
    # a ray batch: the query kernel strides over the batch with the same few workgroups
    q = ds.query_expected(oracle, "deep")
    res = deep.traceRays(q.mix_o, q.mix_d, counters=True)
    assert_hits(res, q.mix_exp)
    assert list(map(int, res["counters"])) == list(map(int, q.mix_cnt))
    assert_hits(deep.traceRays(q.o, q.d), q.exp)
    assert np.array_equal(deep.traceRays(q.a, q.seg_d, any_hit=True)["occluded"], q.occ)
    deep.destroy()
    ctx.close()


@pytest.mark.parametrize("variant", [None, PRIO12, COMPACT], ids=["default", "single-lane", "compact"])
def test_deep_shallow_deep_in_one_context(oracle, variant):
    """The grow-only area and its t plane at cap / 2: a deep frame, a shallow one of another scene, then the
    deep scene again at other sizes and from other views."""
    ctx = beam.Context(device=0, params={} if variant is None else {"trace_variant": variant})
    deep, keep = build(ctx, ds.deep_meshes(0))
    suz_meshes = scenes.load_mesh("suzanne")
    suz, keep2 = build(ctx, suz_meshes)
    err, rays = oracle.camera_rays(*ds.SIZES[0], *ds.CAM)
    assert err == 0
    spacked, stri, st = oracle.bvh_build(suz_meshes, 4, 4).render(rays, (0.0, 0.0, -3.0), scenes.IDENTITY)
    assert 0.05 < float((stri != ds.MISS).mean()) < 0.95
    shallow = (None, None)
    for size, view in ((ds.SIZES[0], "axis"), shallow, (ds.SIZES[1], "mixed"), shallow, (ds.SIZES[0], "diag")):
        if size is None:
            f, _ = trace(ctx, suz, ds.SIZES[0], (0.0, 0.0, -3.0), scenes.IDENTITY)
            assert np.array_equal(f["tri_id"], stri) and np.array_equal(f["packed"], spacked)
            assert np.array_equal(bits(f["t"]), bits(st))
            continue
        e = ds.expected(oracle, "deep", 4, view, size)
        f, cnt = trace(ctx, deep, size, e.eye, e.orient)
        check_frame(f, e, f"{view} {size}")
        assert list(map(int, cnt)) == list(map(int, e.cnt))
    for s in (deep, suz):
        s.destroy()
    ctx.close()


# ---- 5. ray queries ------------------------------------------------------------------------------------
def assert_hits(res, exp, where=None):
    sel = slice(None) if where is None else where
    assert np.array_equal(res["tri_id"][sel], exp["tri_id"][sel]), \
        f"tri_id differs on {int((res['tri_id'][sel] != exp['tri_id'][sel]).sum())} rays"
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(res[k][sel]), bits(exp[k][sel])), k


@pytest.fixture(scope="module", params=ds.QUERY_SCENES)
def qcase(request, oracle):
    name = request.param
    _, dup, leaf = ds.scene_of(name)
    c = beam.Context(device=0, leaf_size=leaf)
    scene, keep = build(c, ds.deep_meshes(dup))
    q = ds.query_expected(oracle, name)
    print(f"{name}: closest-hit batch {ds.fmt(ds.query_stats(q.depth, q.exp['tri_id'] != ds.MISS))}; "
          f"any-hit batch {ds.fmt(ds.query_stats(q.seg_depth, q.occ))}")
    yield name, scene, q
    scene.destroy()
    c.close()


def test_deep_closest_hit_queries(qcase, oracle):
    name, scene, q = qcase
    assert float((q.depth > ds.QUAD_LDS).mean()) >= 0.25
    res = scene.traceRays(q.o, q.d, counters=True)  # 1,999 rays: no multiple of 16
    assert_hits(res, q.exp)
    assert list(map(int, res["counters"])) == list(map(int, q.cnt)), (res["counters"], q.cnt)
    assert_hits(scene.traceRays(q.o, q.d), q.exp)  # the non-counting kernel
    meshes, obvh = ds.oracle_bvh(oracle, name, 4)
    for n in (1, 17):
        sub = {k: v[:n] for k, v in q.exp.items()}
        _, cnt, depth = ds.closest_expected(oracle, obvh, meshes, q.o[:n], q.d[:n])
        assert depth[0] > ds.QUAD_LDS and float((depth > ds.QUAD_LDS).mean()) >= 0.25
        res = scene.traceRays(q.o[:n], q.d[:n], counters=True)
        assert_hits(res, sub)
        assert list(map(int, res["counters"])) == list(map(int, cnt))
        assert_hits(scene.traceRays(q.o[:n], q.d[:n]), sub)


def test_deep_and_shallow_rays_share_a_wave(qcase):
    _, scene, q = qcase
    assert float((q.mix_depth[0::2] > ds.QUAD_LDS).mean()) >= 0.5 and np.all(q.mix_depth[1::2] == 0)
    res = scene.traceRays(q.mix_o, q.mix_d, counters=True)
    assert_hits(res, q.mix_exp)
    assert list(map(int, res["counters"])) == list(map(int, q.mix_cnt))
    assert_hits(scene.traceRays(q.mix_o, q.mix_d), q.mix_exp)


def test_deep_any_hit_queries(qcase, oracle):
    name, scene, q = qcase
    assert float((q.seg_depth > ds.QUAD_LDS).mean()) >= 0.25
    res = scene.traceRays(q.a, q.seg_d, any_hit=True, counters=True)
    assert np.array_equal(res["occluded"], q.occ), f"{int((res['occluded'] != q.occ).sum())} segments differ"
    assert list(map(int, res["counters"])) == list(map(int, q.seg_cnt)), (res["counters"], q.seg_cnt)
    assert np.array_equal(scene.traceRays(q.a, q.seg_d, any_hit=True)["occluded"], q.occ)
    _, obvh = ds.oracle_bvh(oracle, name, 4)
    deep = np.flatnonzero(q.seg_depth > ds.QUAD_LDS)
    for n in (1, 17):  # deep segments only
        sel = deep[:n]
        _, cnt, _ = ds.anyhit_expected(obvh, q.a[sel], q.b[sel])
        res = scene.traceRays(q.a[sel], q.seg_d[sel], any_hit=True, counters=True)
        assert np.array_equal(res["occluded"], q.occ[sel])
        assert list(map(int, res["counters"])) == list(map(int, cnt))
        assert np.array_equal(scene.traceRays(q.a[sel], q.seg_d[sel], any_hit=True)["occluded"], q.occ[sel])


def test_tmax_just_above_and_below_a_deep_hit(qcase):
    _, scene, q = qcase
    hit = np.flatnonzero((q.exp["tri_id"] != ds.MISS) & (q.depth > ds.QUAD_LDS))  # deep rays that hit
    assert hit.size > 100
    t = q.exp["t"][hit]
    above, below = np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(0.0))
    idx = np.tile(hit, 3)
    res = scene.traceRays(q.o[idx], q.d[idx], tmax=np.concatenate([above, t, below]))
    keep = np.arange(2 * hit.size)  # tmax just above t and t itself: the hit
    assert_hits({k: v[keep] for k, v in res.items()}, {k: v[idx[keep]] for k, v in q.exp.items()})
    cut = np.arange(2 * hit.size, 3 * hit.size)  # just below: every other hit is farther
    assert np.all(res["tri_id"][cut] == ds.MISS) and np.all(np.isposinf(res["t"][cut]))
    assert np.all(bits(res["u"][cut]) == 0) and np.all(bits(res["v"][cut]) == 0)


# ---- 6. frames in flight: one overflow area per target stream ------------------------------------------
@pytest.mark.parametrize("variant", [None, COMPACT, PACKET], ids=["default", "compact", "packet"])
def test_deep_frames_in_flight(oracle, variant):
    import torch
    ctx = beam.Context(device=0, params={} if variant is None else {"trace_variant": variant})
    dev = torch.device("cuda", ctx.device)
    scene, keep = build(ctx, ds.deep_meshes(0))
    size = ds.SIZES[0]
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(*size, *ds.CAM) == 0
    exp = [ds.expected(oracle, "deep", 4, view, size) for view in ds.FLIGHT_VIEWS]
    for e in exp:
        deep_enough(e)
    q = ds.query_expected(oracle, "deep")
    n = q.o.shape[0]
    packed = np.zeros((n, 8), np.float32)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = q.o, np.inf, q.d
    rays = torch.from_numpy(packed).to(dev)
    hits = [torch.zeros((n, 4), dtype=torch.float32, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    # serial: one frame at a time on the context stream, and the query alone
    for e in exp:
        f, _ = trace(ctx, scene, size, e.eye, e.orient, counters=False)
        check_frame(f, e, "serial")
    serial = scene.traceRays(q.o, q.d)
    assert_hits(serial, q.exp)
    # in flight: three targets on three streams, three rounds, a deep query on the context stream in between
    streams = [torch.cuda.Stream(device=dev) for _ in exp]
    rts = [beam.IRenderTarget.createOffscreen(ctx, *size) for _ in exp]
    for rt, st in zip(rts, streams):
        rt.setStream(st.cuda_stream)
    for r in range(3):
        for rt, e in zip(rts, exp):
            assert cam.trace(e.eye, e.orient, scene, rt) == 0
        assert scene.traceRaysDevice(rays.data_ptr(), n, hits[r].data_ptr()) == 0
    ctx.sync()
    for rt, e in zip(rts, exp):
        check_frame({k: v.reshape(-1) for k, v in rt.read().items()}, e, "in flight")
    torch.cuda.synchronize()
    for h in hits:
        h = h.cpu().numpy()
        got = {"t": h[:, 0], "u": h[:, 1], "v": h[:, 2], "tri_id": h.view(np.uint32)[:, 3]}
        assert_hits(got, serial)
    # back on the context stream (and its area)
    rts[1].setStream(None)
    assert cam.trace(exp[2].eye, exp[2].orient, scene, rts[1]) == 0
    check_frame({k: v.reshape(-1) for k, v in rts[1].read().items()}, exp[2], "after setStream(None)")
    for rt in rts:
        rt.destroy()
    cam.destroy()
    scene.destroy()
    ctx.close()


# ---- 7. the multi-device path rehearsed on one GPU: two band streams share it --------------------------
def test_deep_frames_over_two_band_streams(oracle):
    ctx = beam.Context(devices=[0, 0])
    scene, keep = build(ctx, ds.deep_meshes(0))
    size = ds.SIZES[0]
    for view in ("axis", "mixed"):
        e = ds.expected(oracle, "deep", 4, view, size)
        f, _ = trace(ctx, scene, size, e.eye, e.orient, counters=False)
        check_frame(f, e, f"{view}")
        e = ds.expected(oracle, "deep", 4, view, size, light=ds.LIGHT)
        f, _ = trace(ctx, scene, size, e.eye, e.orient, light=ds.LIGHT, counters=False)
        check_frame(f, e, f"{view} shadow")
    scene.destroy()
    ctx.close()
