"""GPU parity of ray queries (bm_scene_trace_rays): closest hit and any hit over caller-supplied rays.

The checker is the CPU oracle, unchanged. Closest hit: OrcBVH.render with the identity orientation
traces a ray table from one eye, so a batch is checked group by group (all rays of a group share their
origin); t and tri_id must be bit-equal, u and v bit-equal to orc_pin_ops on the winning triangle (the
same operation sequence), the counters equal to the oracle's summed counters. Any hit: OrcBVH.shadow on
one segment per call (primary t = 0 makes the shadow origin the eye and light - eye the segment).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from raytracercuda_amd import _lib, beam, scenes

pytestmark = pytest.mark.gpu

MISS = np.uint32(0xFFFFFFFF)
GROUPS, PER = 64, 61  # 3,904 rays: no multiple of 16 or 64
ONE_RAY = np.float32([[0.0, 0.0, 1.0]])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def box(meshes):
    pos = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    return lo, hi, (lo + hi) / 2, float(np.linalg.norm(hi - lo))


def tri_vertices(meshes):
    """(ntri, 3, 3) vertex positions by global triangle id (scene order, then face order)."""
    return np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes])


def make_batch(meshes):
    rng = np.random.default_rng(7)
    lo, hi, c, ext = box(meshes)
    o = np.zeros((GROUPS, PER, 3), np.float32)
    d = np.zeros((GROUPS, PER, 3), np.float32)
    for g in range(GROUPS):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        eye = np.float32(c + 0.9 * ext * u)
        targets = np.float32(c + rng.uniform(-0.75, 0.75, (PER, 3)) * (hi - lo))
        o[g] = eye
        d[g] = targets - eye
    return o.reshape(-1, 3), d.reshape(-1, 3) + np.float32(0.0)  # no -0.0 component reaches the oracle


def pin_uv(oracle, o, d, verts, tri):
    """(t, u, v) of orc_pin_ops for ray i against triangle tri[i] (hits only)."""
    fn = oracle.lib.orc_pin_ops
    fn.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    fn.restype = None
    n = o.shape[0]
    rec = np.zeros((n, 36), np.float32)
    rec[:, 0:3] = o
    rec[:, 3:6] = d
    rec[:, 6:15] = scenes.IDENTITY
    rec[:, 15:24] = verts[tri].reshape(n, 9)
    rec[:, 24:33] = np.tile(np.float32([0, 0, 1]), 3)
    out = np.zeros((n, 12), np.float32)
    fn(n, rec.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out[:, 6], out[:, 7], out[:, 8]


def oracle_closest(oracle, obvh, meshes, o, d, per=PER):
    """Expected {t, u, v, tri_id} and summed counters of rays in groups of `per` sharing an origin."""
    n = o.shape[0]
    tri = np.zeros(n, np.uint32)
    t = np.zeros(n, np.float32)
    cnt = np.zeros(3, np.uint64)
    for g in range(0, n, per):
        assert np.all(o[g:g + per] == o[g])
        _, tri[g:g + per], t[g:g + per], c = obvh.render(d[g:g + per], o[g], scenes.IDENTITY, counters=True)
        cnt += c
    hit = tri != MISS
    assert np.all(np.isinf(t[~hit]))
    u = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    if hit.any():
        pt, u[hit], v[hit] = pin_uv(oracle, o[hit], d[hit], tri_vertices(meshes), tri[hit])
        assert np.array_equal(bits(pt), bits(t[hit]))  # the pin restates the trace's triangle test
    return {"t": t, "u": u, "v": v, "tri_id": tri}, cnt


def oracle_anyhit(obvh, o, d_end):
    """Occlusion bytes and summed counters of the segments o[i] -> d_end[i] (one oracle call each)."""
    occ = np.zeros(o.shape[0], np.uint8)
    cnt = np.zeros(3, np.uint64)
    zero_tri, zero_t = np.zeros(1, np.uint32), np.zeros(1, np.float32)
    for i in range(o.shape[0]):
        s, c = obvh.shadow(ONE_RAY, o[i], scenes.IDENTITY, d_end[i], zero_tri, zero_t, counters=True)
        occ[i] = s[0]
        cnt += c
    return occ, cnt


def assert_hits(res, exp, where=None):
    sel = slice(None) if where is None else where
    assert np.array_equal(res["tri_id"][sel], exp["tri_id"][sel]), \
        f"tri_id differs on {int((res['tri_id'][sel] != exp['tri_id'][sel]).sum())} rays"
    for k in ("t", "u", "v"):
        assert np.array_equal(bits(res[k][sel]), bits(exp[k][sel])), k


def segments(meshes, n=1500):
    rng = np.random.default_rng(11)
    lo, hi, c, _ = box(meshes)
    a = np.float32(c + rng.uniform(-0.75, 0.75, (n, 3)) * (hi - lo))
    b = np.float32(c + rng.uniform(-0.75, 0.75, (n, 3)) * (hi - lo))
    return a, b, np.float32(b) - np.float32(a)


def build(ctx, meshes):
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    return scene, keep


_CASES = {}


def case(ctx, oracle, name):
    """Mesh, GPU scene, the parity batch and the oracle's answers for it — computed once per module run."""
    if name not in _CASES:
        meshes = scenes.load_mesh(name)
        scene, keep = build(ctx, meshes)
        obvh = oracle.bvh_build(meshes, 4, 4)
        o, d = make_batch(meshes)
        exp, cnt = oracle_closest(oracle, obvh, meshes, o, d)
        _CASES[name] = SimpleNamespace(meshes=meshes, scene=scene, keep=keep, obvh=obvh, o=o, d=d, exp=exp, cnt=cnt)
    return _CASES[name]


@pytest.fixture(scope="module")
def suz_segments(ctx, oracle):
    k = case(ctx, oracle, "suzanne")
    a, b, d = segments(k.meshes)
    occ, cnt = oracle_anyhit(k.obvh, a, b)
    return SimpleNamespace(a=a, b=b, d=d, occ=occ, cnt=cnt)


# ---- 1. parity on meshes -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["suzanne", "bunny"])
def test_closest_parity_with_the_oracle(ctx, oracle, name):
    k = case(ctx, oracle, name)
    frac = float((k.exp["tri_id"] != MISS).mean())
    assert 0.1 <= frac <= 0.9, frac
    res = k.scene.traceRays(k.o, k.d, counters=True)
    assert_hits(res, k.exp)
    assert list(map(int, res["counters"])) == list(map(int, k.cnt)), (res["counters"], k.cnt)
    plain = k.scene.traceRays(k.o, k.d)  # the non-counting kernel
    assert_hits(plain, k.exp)


# ---- 2. batch edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 15, 16, 17, 63, 64, 65, 1025])
def test_batch_edges_write_nothing_past_n(ctx, oracle, suz_segments, n):
    import torch
    k = case(ctx, oracle, "suzanne")
    dev = torch.device("cuda", ctx.device)
    rays = np.zeros((max(n, 1), 8), np.float32)
    rays[:n, 0:3], rays[:n, 3], rays[:n, 4:7] = k.o[:n], np.inf, k.d[:n]
    segs = np.zeros((max(n, 1), 8), np.float32)
    segs[:n, 0:3], segs[:n, 4:7] = suz_segments.a[:n], suz_segments.d[:n]
    hits = torch.full((n + 64, 4), -7.5, dtype=torch.float32, device=dev)
    occ = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=dev)
    r_dev, s_dev = torch.from_numpy(rays).to(dev), torch.from_numpy(segs).to(dev)
    torch.cuda.synchronize()
    assert k.scene.traceRaysDevice(r_dev.data_ptr(), n, hits.data_ptr()) == 0
    assert k.scene.traceRaysDevice(s_dev.data_ptr(), n, occ.data_ptr(), any_hit=True) == 0
    ctx.sync()
    h, oc = hits.cpu().numpy(), occ.cpu().numpy()
    assert np.all(h[n:] == np.float32(-7.5)) and np.all(oc[n:] == 0xAB)
    got = {"t": h[:n, 0], "u": h[:n, 1], "v": h[:n, 2], "tri_id": h.view(np.uint32)[:n, 3]}
    assert_hits(got, {key: val[:n] for key, val in k.exp.items()})
    assert np.array_equal(oc[:n], suz_segments.occ[:n])


# ---- 3. grid stride ----------------------------------------------------------------------------------
def test_small_grid_strides_over_the_batches(oracle, ctx):
    k = case(ctx, oracle, "suzanne")
    small = beam.Context(device=0, params={"trace_grid": 2})  # 8 waves: about 30 batches each
    scene, keep = build(small, k.meshes)
    assert_hits(scene.traceRays(k.o, k.d), k.exp)
    scene.destroy()
    small.close()


# ---- 4. tmax -----------------------------------------------------------------------------------------
def test_tmax_bounds_the_hit(ctx, oracle):
    k = case(ctx, oracle, "suzanne")
    hit = np.flatnonzero(k.exp["tri_id"] != MISS)
    t = k.exp["t"][hit]
    zero = np.float32(0.0)
    tmax = np.concatenate([np.full(hit.size, np.inf, np.float32), t, np.nextafter(t, zero), np.float32(0.5) * t])
    idx = np.tile(hit, 4)
    res = k.scene.traceRays(k.o[idx], k.d[idx], tmax=tmax)
    keep = np.arange(2 * hit.size)  # tmax = inf and tmax = t: the hit itself
    assert_hits({key: val[keep] for key, val in res.items()}, {key: val[idx[keep]] for key, val in k.exp.items()})
    cut = np.arange(2 * hit.size, 4 * hit.size)  # just below t and half of it: every other hit is farther
    assert np.all(res["tri_id"][cut] == MISS) and np.all(np.isposinf(res["t"][cut]))
    assert np.all(bits(res["u"][cut]) == 0) and np.all(bits(res["v"][cut]) == 0)


# ---- 5. tiny scenes against brute force --------------------------------------------------------------
@pytest.mark.parametrize("ntri", [0, 1, 2, 5, 17])
def test_tiny_scenes_against_exhaustive(ctx, oracle, ntri):
    rng = np.random.default_rng(100 + ntri)
    pos = rng.uniform(-1, 1, (3 * ntri, 3)).astype(np.float32)
    pos[:, 2] = rng.uniform(0.0, 2.0, 3 * ntri).astype(np.float32)
    meshes = [{"pos": pos, "nrm": np.tile(np.float32([0, 0, 1]), (3 * ntri, 1)),
               "idx": np.arange(3 * ntri, dtype=np.uint32)}] if ntri else []
    scene, keep = build(ctx, meshes)
    eyes = np.float32(rng.uniform(-2, 2, (8, 3)))
    targets = np.float32(rng.uniform([-1, -1, 0], [1, 1, 2], (8, 37, 3)))
    o = np.repeat(eyes, 37, axis=0)
    d = (targets - eyes[:, None, :]).reshape(-1, 3) + np.float32(0.0)
    a = np.float32(rng.uniform([-1.5, -1.5, -0.5], [1.5, 1.5, 2.5], (200, 3)))
    b = np.float32(rng.uniform([-1.5, -1.5, -0.5], [1.5, 1.5, 2.5], (200, 3)))
    res = scene.traceRays(o, d)
    occ = scene.traceRays(a, b - a, any_hit=True)["occluded"]
    if ntri == 0:
        assert np.all(res["tri_id"] == MISS) and np.all(np.isposinf(res["t"])) and not occ.any()
        scene.destroy()
        return
    for g in range(8):
        _, tri, t = oracle.brute_render(meshes, d[37 * g:37 * g + 37], eyes[g], scenes.IDENTITY)
        assert np.array_equal(res["tri_id"][37 * g:37 * g + 37], tri)
        assert np.array_equal(bits(res["t"][37 * g:37 * g + 37]), bits(t))
    exp = np.array([oracle.brute_shadow(meshes, ONE_RAY, a[i], scenes.IDENTITY, b[i], np.zeros(1, np.uint32),
                                        np.zeros(1, np.float32))[0] for i in range(200)], np.uint8)
    assert np.array_equal(occ, exp)
    scene.destroy()


# ---- 6. any-hit parity -------------------------------------------------------------------------------
def test_any_hit_parity_with_the_oracle(ctx, oracle, suz_segments):
    k = case(ctx, oracle, "suzanne")
    s = suz_segments
    frac = float(s.occ.mean())
    assert 0.1 <= frac <= 0.9, frac
    res = k.scene.traceRays(s.a, s.d, any_hit=True, counters=True)
    assert np.array_equal(res["occluded"], s.occ)
    assert list(map(int, res["counters"])) == list(map(int, s.cnt)), (res["counters"], s.cnt)
    # tmax is ignored in this mode, and the non-counting kernel agrees
    plain = k.scene.traceRays(s.a, s.d, tmax=np.float32(1e-3), any_hit=True)
    assert np.array_equal(plain["occluded"], s.occ)


# ---- 7. axis-parallel and invalid rays ---------------------------------------------------------------
def test_axis_parallel_and_invalid_rays(ctx, oracle):
    k = case(ctx, oracle, "suzanne")
    n = k.o.shape[0]
    o, d = k.o.copy(), k.d.copy()
    tmax = np.full(n, np.inf, np.float32)
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
    # the oracle sees the valid rays only (origins unchanged there: the groups still share theirs)
    od = np.where(invalid[:, None], k.d, d)
    exp, cnt = oracle_closest(oracle, k.obvh, k.meshes, k.o, od)
    axis = sel[kind <= 1]
    changed = np.zeros(n, bool)
    changed[sel] = True
    assert_hits(exp, k.exp, ~changed)  # every ray that was not replaced keeps test 1's result
    for i in np.flatnonzero(invalid):  # invalid rays count nothing: take their stand-ins' share out
        cnt -= k.obvh.render(k.d[i:i + 1], k.o[i], scenes.IDENTITY, counters=True)[3]
    res = k.scene.traceRays(o, d, tmax=tmax, counters=True)
    assert_hits(res, exp, ~invalid)
    assert np.all(res["tri_id"][invalid] == MISS) and np.all(np.isposinf(res["t"][invalid]))
    assert np.all(bits(res["u"][invalid]) == 0) and np.all(bits(res["v"][invalid]) == 0)
    assert list(map(int, res["counters"])) == list(map(int, cnt)), (res["counters"], cnt)
    occ = k.scene.traceRays(o, d, tmax=tmax, any_hit=True)["occluded"]
    base = k.scene.traceRays(k.o, k.d, any_hit=True)["occluded"]
    geo_invalid = np.zeros(n, bool)
    geo_invalid[sel[(kind == 2) | (kind == 3)]] = True
    assert not occ[geo_invalid].any()
    same = ~changed
    same[sel[kind >= 4]] = True  # tmax does not make a ray invalid in any-hit mode
    assert np.array_equal(occ[same], base[same])
    exp_axis, _ = oracle_anyhit(k.obvh, o[axis], o[axis] + d[axis])
    # the segment's end is the oracle's input: keep the rays whose end reproduces d exactly
    exact = np.all((o[axis] + d[axis]) - o[axis] == d[axis], axis=1)
    assert exact.sum() > 10
    assert np.array_equal(occ[axis][exact], exp_axis[exact])


# ---- 8. refit ----------------------------------------------------------------------------------------
def test_query_after_refit(ctx, oracle):
    k = case(ctx, oracle, "bunny")
    scene = beam.IScene.create(ctx)
    meshes = beam.upload_meshes(ctx, scene, k.meshes)
    scene.updateGPUScene()
    moved = []
    for m in k.meshes:
        p = np.asarray(m["pos"], np.float32)
        q = p.copy()
        q[:, 1] += np.float32(0.03) * np.sin(np.float32(8.0) * p[:, 0] + np.float32(1.0)).astype(np.float32)
        q[:, 0] += np.float32(0.009) * np.cos(np.float32(5.0) * p[:, 2]).astype(np.float32)
        moved.append(dict(m, pos=q))
    for m, mv in zip(meshes, moved):
        assert m.setVertexData(mv["pos"], mv["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    obvh = oracle.bvh_build(k.meshes, 4, 4).refit(moved)
    n = 8 * PER
    exp, cnt = oracle_closest(oracle, obvh, moved, k.o[:n], k.d[:n])
    assert (exp["tri_id"] != MISS).any() and not np.array_equal(exp["tri_id"], k.exp["tri_id"][:n])
    res = scene.traceRays(k.o[:n], k.d[:n], counters=True)
    assert_hits(res, exp)
    assert list(map(int, res["counters"])) == list(map(int, cnt))
    scene.destroy()


# ---- 9. errors ---------------------------------------------------------------------------------------
def test_errors(ctx, oracle):
    import torch
    k = case(ctx, oracle, "suzanne")
    dev = torch.device("cuda", ctx.device)
    n = 64
    rays = torch.zeros((n + 1, 8), dtype=torch.float32, device=dev)
    out = torch.zeros((n + 1, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rp, op = rays.data_ptr(), out.data_ptr()
    bad = _lib.ERROR_INVALID_PARAMETER
    unbuilt = beam.IScene.create(ctx)
    assert unbuilt.traceRaysDevice(rp, n, op) == _lib.ERROR_NOT_BUILT
    unbuilt.destroy()
    s = k.scene
    assert s.traceRaysDevice(rp, n, op) == 0
    assert s.traceRaysDevice(0, n, op) == bad and s.traceRaysDevice(rp, n, 0) == bad
    assert s.traceRaysDevice(0, 0, 0) == 0  # n = 0: nothing to read or write
    off_r, off_o = rays.view(-1)[1:].data_ptr(), out.view(-1)[1:].data_ptr()  # 4 bytes in
    assert off_r == rp + 4 and off_o == op + 4
    assert s.traceRaysDevice(off_r, n, op) == bad and s.traceRaysDevice(rp, n, off_o) == bad
    assert s.traceRaysDevice(rp, n, off_o, any_hit=True) == bad
    assert s.traceRaysDevice(rp, n, op, mode=2) == bad
    for flags in (1, 2, 0x80000000):  # no flag bits are defined
        assert s.traceRaysDevice(rp, n, op, flags=flags) == bad
        assert s.traceRaysDevice(rp, n, op, any_hit=True, flags=flags) == bad
    cnt = np.zeros(3, np.uint64)
    assert s.traceRaysDevice(rp, n, op, mode=7, counters=cnt) == bad
    ctx.sync()
    tiny = [{"pos": np.float32([[0, 0, 1], [1, 0, 1], [0, 1, 1]]), "nrm": np.float32([[0, 0, 1]] * 3),
             "idx": np.uint32([0, 1, 2])}]
    for kw in ({"reference_kd": True}, {"reference_hash": True}, {"bvh_width": 2}):
        other = beam.Context(device=0, **kw)
        sc, keep = build(other, tiny)
        assert sc.traceRaysDevice(rp, n, op) == bad, kw
        assert sc.traceRaysDevice(rp, n, op, any_hit=True) == bad, kw
        sc.destroy()
        other.close()


def test_rehearsal_context_queries_on_the_root(ctx, oracle):
    k = case(ctx, oracle, "suzanne")
    multi = beam.Context(devices=[0, 0])
    scene, keep = build(multi, k.meshes)
    assert_hits(scene.traceRays(k.o, k.d), k.exp)
    scene.destroy()
    multi.close()


# ---- 10. torch path ----------------------------------------------------------------------------------
def test_torch_tensors_stay_on_the_device_and_chain(ctx, oracle):
    import torch
    k = case(ctx, oracle, "suzanne")
    dev = torch.device("cuda", 0)
    tctx = beam.Context(device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    scene, keep = build(tctx, k.meshes)
    n = k.o.shape[0]
    packed = np.zeros((n, 8), np.float32)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = k.o, np.inf, k.d
    rays = torch.from_numpy(packed).to(dev)
    light = torch.tensor([1.5, 2.0, -2.5], dtype=torch.float32, device=dev)
    # no synchronisation from here to the end of the chain
    res = scene.traceRays(rays)
    assert res["hits"].is_cuda and res["hits"].shape == (n, 4) and res["tri_id"].dtype == torch.int32
    o2 = rays[:, 0:3] + rays[:, 4:7] * (res["t"] * 0.9999)[:, None]
    d2 = light[None, :] - o2
    occ = scene.traceRays(o2, d2, any_hit=True)["occluded"]
    assert occ.is_cuda and occ.dtype == torch.uint8 and occ.shape == (n,)
    split = scene.traceRays(rays[:, 0:3].contiguous(), rays[:, 4:7].contiguous())
    torch.cuda.synchronize()
    got = {key: res[key].cpu().numpy() for key in ("t", "u", "v")}
    got["tri_id"] = res["tri_id"].cpu().numpy().view(np.uint32)
    assert_hits(got, k.exp)
    assert torch.equal(split["hits"].view(torch.int32), res["hits"].view(torch.int32))
    # the chained segments against the oracle, from the very origins and ends the device computed
    hit = k.exp["tri_id"] != MISS
    o2h, occ_h = o2.cpu().numpy(), occ.cpu().numpy()
    assert not occ_h[~hit].any()  # a miss has t = inf: a non-finite origin, finished unoccluded
    idx = np.flatnonzero(hit)
    lh = np.broadcast_to(light.cpu().numpy(), (idx.size, 3))
    assert np.array_equal(bits(d2.cpu().numpy()[idx]), bits(lh - o2h[idx]))
    exp_occ, _ = oracle_anyhit(k.obvh, o2h[idx], np.ascontiguousarray(lh))
    assert np.array_equal(occ_h[idx], exp_occ)
    assert 0 < exp_occ.sum() < idx.size
    scene.destroy()
    tctx.close()


def teardown_module(module):
    for k in _CASES.values():
        k.scene.destroy()
    _CASES.clear()
