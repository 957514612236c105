"""The compacted trace (k_cull + k_trace_rays) at the edges of its ray queue.

k_cull lays the frame out in regions of BM_PARAM_CULL_TILES 8x8 tiles (trace_compact_layout: a multiple of 4,
grown by 4 until at most 1,024 regions remain) and appends each region's surviving rays to its part of the
queue; k_trace_rays finds every 16-ray batch's region by a 64-ary ballot search over an LDS prefix of the
region counts and lets each ray step forward over the region ends inside its batch. A wrong step is a missing
or a doubled ray, so every case compares ids, packed colours and t bit for bit with the oracle's frame and the
node, triangle and hit counters with the oracle's, and the region counts the GPU wrote with the bounds the
oracle's root record allows (survivor_bounds).

Frames (at 4 tiles per region): 1, 15, 16 and 17 regions; a ragged frame; exactly 1,024 regions; 4,160 and
8,320 tiles, which grow the region to 8 and 12 tiles; 20 and 36 tiles per region, whose last unroll step of
k_cull is partial; 65535 x 8, the widest frame the 16-bit pixel packing takes. Scenes: (a) a dense view, (b)
"specks", 1 to 15 surviving rays in regions hundreds apart, (c) a mirrored orient and (e) the empty scene,
where no ray survives, and (d) "wire", a thin steep diagonal whose survivors come a few per region, so that
batches of 16 span several regions, the last region among them. What (b) and (d) must give the queue is
asserted from the oracle's root record alone (test_scene_conditions).

test_frames_beyond_the_pixel_packing: 65536 x 4 and 4 x 65536 cannot be packed (x | lr << 16) and take the
quad kernel. Before this file they fell through to the packet kernel instead, which trace_impl had not
prepared for: it reported "quads", and no envelope check kept the far eye from it. Run against a library with
that defect put back, all four cases passed: neither the near nor the far eye's frame would have caught it, on
either frame shape. The fix was made by reading launch_variant; the test pins the frames and the reported
kind of the fallback. The parameter bound of test_cull_tiles_bounds is what a test does catch: without the
cap the three refused values are accepted.

Measured on an MI355X: run alone the file takes 14.8 s of wall time (72 tests), 11 s of it PyTorch's start
for the one HIP stream of test_automatic_choice_with_cull_tiles, which the whole suite pays once elsewhere; the
largest case takes a third of a second, the oracle's frame on the CPU included.
"""
import numpy as np
import pytest

from raytracercuda_amd import beam, scenes
from test_gpu_variants import check, expect

pytestmark = pytest.mark.gpu

QUAD, COMPACT = 10, 12
CULL_TILE, MAX_REGIONS = 8, 1024  # bm_trace_quad.h
EYE = (0.1, 0.05, -3.0)
LIGHT = (0.0, 10.0, -10.0)
CAM = scenes.RAYS_SQUARE
MIRRORED = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0)  # test_variant_general_orient: looking away


def _soup(pos):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    nrm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (pos.shape[0], 1))
    return [{"pos": pos, "nrm": nrm, "idx": np.arange(pos.shape[0], dtype=np.uint32)}]


def dense_scene():
    """(a) 40 random triangles (test_variant_ragged_frames' scene)."""
    rng = np.random.default_rng(4021)
    n = 40
    return [{"pos": rng.uniform(-1, 1, size=(3 * n, 3)).astype(np.float32),
             "nrm": rng.normal(size=(3 * n, 3)).astype(np.float32), "idx": np.arange(3 * n, dtype=np.uint32)}]


def pixel_at(px, py, n=512, z=0.0):
    """World point on the plane z through which the centre ray of pixel (px, py) of an n x n frame passes."""
    s = (z - EYE[2])
    return np.array([EYE[0] + (-1.0 + (px + 0.5) * 2.0 / n) * s, EYE[1] + (-1.0 + (py + 0.5) * 2.0 / n) * s, z])


def specks_scene():
    """(b) 16 triangles a third of a 512 x 512 frame's pixel across, four around each of four pixel centres
    in the frame's four quadrants: every root child is one cluster's leaf."""
    rng = np.random.default_rng(11)
    tris = []
    for px, py in ((21, 10), (403, 41), (100, 301), (490, 501)):
        c = pixel_at(px, py)
        for _ in range(4):
            tris.append(c + rng.uniform(-0.002, 0.002, size=(3, 3)) * (1, 1, 0.25))
    return _soup(np.concatenate(tris))


def wire_scene():
    """(d) 200 small triangles along a thin, steep diagonal of the 512 x 512 frame: down pixel column 493 from
    row 3 to row 511, drifting a tenth of a pixel. The root's children are tall boxes a third of a pixel
    wide, so each 8-row tile they cross holds at most 8 survivors, and they end in the last region."""
    rng = np.random.default_rng(12)
    n = 200
    tris = []
    for k in range(n):
        a = (k + 0.5) / n
        c = pixel_at(493.0 + 0.1 * (a - 0.5), 3.0 + 508.0 * a)
        tris.append(c + rng.uniform(-1, 1, size=(3, 3)) * (0.0012, 0.012, 0.001))
    return _soup(np.concatenate(tris))


SCENES = {"dense": dense_scene(), "specks": specks_scene(), "wire": wire_scene(), "empty": []}
_expected, _bounds = {}, {}


def expected(oracle, scene, w, h, eye=EYE, orient=None, light=None, cam=CAM):
    """The oracle's frame and counters, computed once per view and shared (never modified)."""
    orient = scenes.IDENTITY if orient is None else np.asarray(orient, np.float32)
    key = (scene, w, h, tuple(eye), tuple(orient), light, tuple(cam))
    if key not in _expected:
        _expected[key] = expect(oracle, SCENES[scene], w, h, cam, eye, orient, light=light)
    return _expected[key]


def layout(w, h, min_tpr):
    """trace_compact_layout (bm_trace.hip): (regions, tiles per region), None when the frame cannot be packed."""
    if w > 0xFFFF or h > 0xFFFF:
        return None
    ntiles = ((w + CULL_TILE - 1) // CULL_TILE) * ((h + CULL_TILE - 1) // CULL_TILE)
    tpr = (min_tpr + 3) // 4 * 4 if min_tpr and min_tpr >= 4 else 32
    while (ntiles + tpr - 1) // tpr > MAX_REGIONS:
        tpr += 4
    return (ntiles + tpr - 1) // tpr, tpr


def survivor_bounds(oracle, scene, w, h, eye=EYE, orient=None, cam=CAM):
    """(sure, maybe): bool [h, w] masks of the rays that must and that may survive k_cull, from the oracle's
    root record alone. k_cull keeps a ray that enters one of the root's four child boxes inflated by
    m = 2^-12 x max(|eye|, |box coordinates|); its slab distances deviate from exact ones by far less than m.
    In float64: a ray that enters a box inflated by m - 2m must survive, one that misses every box inflated by
    m + 2m must not, and the rays between count to neither side. A direction with a component below 2^-100
    is never culled."""
    key = (scene, w, h, tuple(eye), None if orient is None else tuple(orient), tuple(cam))
    if key not in _bounds:
        _bounds[key] = _survivor_bounds(oracle, scene, w, h, eye, orient, cam)
    return _bounds[key]


def _survivor_bounds(oracle, scene, w, h, eye, orient, cam):
    if not SCENES[scene]:
        z = np.zeros((h, w), bool)
        return z, z
    orient = np.asarray(scenes.IDENTITY if orient is None else orient, np.float64).reshape(3, 3)  # [col][row]
    root = oracle.bvh_build(SCENES[scene], 4, 4).export()[0][0].view(np.float32).astype(np.float64)
    lo, hi = root[0:12].reshape(3, 4), root[12:24].reshape(3, 4)  # word 4 * axis + child
    kids = ~np.isnan(lo[0])
    e = np.asarray(eye, np.float64)
    m = 2.0 ** -12 * max(np.abs(e).max(), np.abs(lo[:, kids]).max(), np.abs(hi[:, kids]).max())
    err, rays = oracle.camera_rays(w, h, *cam)
    assert err == 0
    d = rays.astype(np.float64) @ orient  # dir[row] = sum over col of orient[col][row] * ray[col]
    tiny = (np.abs(d) < 2.0 ** -100).any(axis=1)

    def enters(grow):
        any_hit = np.zeros(d.shape[0], bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            for k in np.nonzero(kids)[0]:
                t0 = (lo[:, k] - grow - e) / d
                t1 = (hi[:, k] + grow - e) / d
                tn = np.minimum(t0, t1).max(axis=1)
                tf = np.maximum(t0, t1).min(axis=1)
                any_hit |= (tn <= tf) & (tf >= 0)
        return any_hit

    sure = (enters(-m) | tiny).reshape(h, w)
    maybe = (enters(3 * m) | tiny).reshape(h, w)
    return sure, maybe | sure


def region_counts(mask, tpr):
    """Rays of a bool [h, w] mask per queue region of tpr tiles (tiles in row-major order)."""
    h, w = mask.shape
    tx, ty = (w + CULL_TILE - 1) // CULL_TILE, (h + CULL_TILE - 1) // CULL_TILE
    pad = np.zeros((ty * CULL_TILE, tx * CULL_TILE), np.int64)
    pad[:h, :w] = mask
    tiles = pad.reshape(ty, CULL_TILE, tx, CULL_TILE).sum(axis=(1, 3)).reshape(-1)
    regions = (tiles.size + tpr - 1) // tpr
    return np.bincount(np.arange(tiles.size) // tpr, weights=tiles, minlength=regions).astype(np.int64)


def batch_spans(counts):
    """For every 16-ray batch of the concatenated queue: regions from its first ray's to its last ray's."""
    pre = np.cumsum(counts)
    total = int(pre[-1]) if pre.size else 0
    first = np.arange(0, total, 16)
    last = np.minimum(first + 15, total - 1)
    return np.searchsorted(pre, last, side="right") - np.searchsorted(pre, first, side="right") + 1


def test_scene_conditions(oracle):
    """What scenes (b) and (d) must give the queue at 512 x 512 and 4 tiles per region, by the oracle alone."""
    assert layout(512, 512, 4) == (1024, 4) and layout(520, 512, 4) == (520, 8) and layout(1024, 520, 4)[1] == 12
    assert [layout(w, h, 4)[0] for w, h in ((8, 8), (80, 48), (64, 64), (136, 32))] == [1, 15, 16, 17]
    assert layout(65535, 8, 4) == (1024, 8) and layout(65536, 4, 4) is None and layout(4, 65536, 4) is None
    # (b): between 1 and 15 survivors, in at least 3 different regions
    sure, maybe = survivor_bounds(oracle, "specks", 512, 512)
    assert 1 <= sure.sum() and maybe.sum() <= 15, (sure.sum(), maybe.sum())
    assert (region_counts(sure, 4) > 0).sum() >= 3
    # (d): at least 30 regions of 1 to 15 survivors, at least 10 batches spanning 3 or more regions, and rays
    # in the last region that share a batch with an earlier region's (whichever way the undecided rays fall)
    sure, maybe = survivor_bounds(oracle, "wire", 512, 512)
    lo, hi = region_counts(sure, 4), region_counts(maybe, 4)
    assert ((lo >= 1) & (hi <= 15)).sum() >= 30, ((lo >= 1) & (hi <= 15)).sum()
    for c in (lo, hi):
        spans = batch_spans(c)
        assert (spans >= 3).sum() >= 10, (spans >= 3).sum()
        assert c[-1] > 0 and spans[-1] >= 3
    # (c), (e): no survivor at all; (a): a solid block of the frame, thousands of batches at 512 x 512
    assert survivor_bounds(oracle, "dense", 130, 67, orient=MIRRORED)[1].sum() == 0
    assert survivor_bounds(oracle, "dense", 130, 67)[0].mean() > 0.1


_ctxs = {}


@pytest.fixture(scope="module")
def cctx():
    """Contexts on the compacted path (sched 1), one per (cull_tiles, trace_grid), shared by the module."""

    def get(cull_tiles=None, grid=None):
        key = (cull_tiles, grid)
        if key not in _ctxs:
            params = {"trace_variant": COMPACT, "trace_sched": 1}
            if cull_tiles is not None:
                params["cull_tiles"] = cull_tiles
            if grid is not None:
                params["trace_grid"] = grid
            _ctxs[key] = beam.Context(device=0, params=params)
        return _ctxs[key]

    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


def render(ctx, scene, w, h, eye=EYE, orient=None, light=None, cam=CAM, stream=None):
    """test_gpu_variants.render, which also returns the kernels that ran and the queue's region counts."""
    orient = scenes.IDENTITY if orient is None else np.asarray(orient, np.float32)
    sc = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, sc, SCENES[scene])
    sc.updateGPUScene()
    ctx.sync()
    c = beam.ICamera.create(ctx)
    assert c.setInitialRays(w, h, *cam) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, w, h)
    if stream is not None:
        rt.setStream(stream)
    if light is None:
        cnt = c.traceCounters(eye, orient, sc, rt)
        assert c.trace(eye, orient, sc, rt) == 0
    else:
        cnt = c.traceShadowCounters(eye, orient, sc, rt, light)
        assert c.traceShadow(eye, orient, sc, rt, light) == 0
    f = {k: v.reshape(-1) for k, v in rt.read().items()}
    if light is not None:
        f["shadow"] = rt.readShadow().reshape(-1)
    kind = rt.traceKind()
    counts = rt.rayQueueCounts() if kind == "cull+quads" else None
    rt.destroy()
    c.destroy()
    sc.destroy()
    del keep
    return f, cnt, kind, counts


def run_case(ctx, oracle, scene, w, h, cull_tiles, orient=None, light=None, stream=None):
    f, cnt, kind, counts = render(ctx, scene, w, h, orient=orient, light=light, stream=stream)
    assert kind == "cull+quads"
    regions, tpr = layout(w, h, cull_tiles)
    assert counts.shape == (regions,)
    sure, maybe = survivor_bounds(oracle, scene, w, h, orient=orient)
    lo, hi = region_counts(sure, tpr), region_counts(maybe, tpr)
    bad = np.nonzero((counts < lo) | (counts > hi))[0]
    assert bad.size == 0, f"region counts outside the oracle's bounds at regions {bad[:8]}"
    check(f, cnt, *expected(oracle, scene, w, h, orient=orient, light=light))
    return counts


FRAMES = [(8, 8), (80, 48), (64, 64), (136, 32), (130, 67), (512, 512), (520, 512), (1024, 520)]
SPARSE_FRAMES = [(8, 8), (130, 67), (512, 512), (1024, 520)]
CASES = ([("dense", w, h, 4, None) for w, h in FRAMES] + [("wire", w, h, 4, None) for w, h in FRAMES] +
         [("specks", w, h, 4, None) for w, h in SPARSE_FRAMES] + [("empty", w, h, 4, None) for w, h in SPARSE_FRAMES] +
         [("dense", w, h, 4, MIRRORED) for w, h in SPARSE_FRAMES] +
         [(s, w, h, t, None) for t in (None, 8, 20, 32, 36, 1024, 65536) for s in ("dense", "wire")
          for w, h in ((130, 67), (512, 512))] +
         [("specks", 512, 512, t, None) for t in (None, 20, 36)])


@pytest.mark.parametrize("scene,w,h,cull_tiles,orient", CASES,
                         ids=[f"{s}{'-mirrored' if o else ''}-{w}x{h}-tiles{t}" for s, w, h, t, o in CASES])
def test_frames_and_counters(cctx, oracle, scene, w, h, cull_tiles, orient):
    counts = run_case(cctx(cull_tiles), oracle, scene, w, h, cull_tiles, orient=orient)
    if scene == "empty" or orient is not None:
        assert counts.sum() == 0
    if scene == "specks" and (w, h) == (512, 512):
        assert 1 <= counts.sum() <= 15


@pytest.mark.parametrize("grid", [1, 3, 12])
def test_small_grids(cctx, oracle, grid):
    """One, three and twelve workgroups walk every batch of (d)'s queue."""
    run_case(cctx(4, grid), oracle, "wire", 512, 512, 4)


def test_fused_shadow(cctx, oracle):
    run_case(cctx(4), oracle, "dense", 130, 67, 4, light=LIGHT)
    run_case(cctx(4), oracle, "wire", 512, 512, 4, light=LIGHT)


def test_bands(cctx, oracle):
    """16-row bands dealt to 3 ranks: local rows are packed into the queue and mapped back by global_row."""
    ctx = cctx(4)
    w, h, bh, n = 130, 67, 16, 3
    exp, _ = expected(oracle, "dense", w, h)
    sc = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, sc, SCENES["dense"])
    sc.updateGPUScene()
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(w, h, *CAM) == 0
    bands = (h + bh - 1) // bh
    for r in range(n):
        mine = [b for b in range(bands) if b % n == r]
        rt = beam.IRenderTarget.createOffscreen(ctx, w, len(mine) * bh)
        assert cam.traceBands(EYE, scenes.IDENTITY, sc, rt, bh, n, r) == 0
        assert rt.traceKind() == "cull+quads"
        part = rt.read()
        rt.destroy()
        for i, b in enumerate(mine):
            rows = slice(b * bh, min((b + 1) * bh, h))
            k = rows.stop - rows.start
            for plane in ("packed", "tri_id", "t"):
                got = part[plane][i * bh:i * bh + k].view(np.uint32)
                assert np.array_equal(got, exp[plane].reshape(h, w)[rows].view(np.uint32)), f"rank {r} band {b} {plane}"
    cam.destroy()
    sc.destroy()
    del keep


def test_automatic_choice_with_cull_tiles(oracle):
    """The default context picks the compacted trace for a target on its own stream over a sparse view;
    cull_tiles lays its queue out as for the forced variant."""
    import torch

    ctx = beam.Context(device=0, params={"cull_tiles": 4})
    try:
        assert ctx.get_param("trace_variant") == -1
        st = torch.cuda.Stream()
        run_case(ctx, oracle, "wire", 512, 512, 4, stream=st.cuda_stream)
    finally:
        ctx.close()


def test_widest_packed_frame(cctx, oracle):
    """65535 x 8: x = 65534 still fits the 16-bit packing; 8,192 tiles grow the region to 8."""
    run_case(cctx(4), oracle, "dense", 65535, 8, 4)


FAR = 4096 * 2.0  # 4,096 extents of the dense scene (side 2) from its centre


@pytest.mark.parametrize("w,h", [(65536, 4), (4, 65536)])
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
def test_frames_beyond_the_pixel_packing(cctx, oracle, w, h, far):
    """No ray queue: the quad kernel, reported as such, from a near eye and from one 4,096 extents away (a
    window narrowed by as much keeps the scene in view). Of the two defects fixed with this file, the test
    would have caught neither by its frames: with the fall-through to the packet kernel put back, the near
    and the far eye's frames still equalled the oracle's on both shapes (measured). The missing cap on
    cull_tiles is caught by test_cull_tiles_bounds."""
    eye = (0.1, 0.05, -FAR) if far else EYE
    cam = tuple(float(np.float32(v * 1.2 / FAR)) for v in CAM[:4]) + (1.0,) if far else CAM
    orient = scenes.IDENTITY
    ctx = cctx(4)
    sc = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, sc, SCENES["dense"])
    sc.updateGPUScene()
    ctx.sync()
    c = beam.ICamera.create(ctx)
    assert c.setInitialRays(w, h, *cam) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, w, h)
    cnt = c.traceCounters(eye, orient, sc, rt)
    assert c.trace(eye, orient, sc, rt) == 0
    kind = rt.traceKind()
    f = {k: v.reshape(-1) for k, v in rt.read().items()}
    rt.destroy()
    c.destroy()
    sc.destroy()
    del keep
    assert kind == "quads"
    exp, ecnt = expected(oracle, "dense", w, h, eye=eye, cam=cam)
    assert (exp["tri_id"] != 0xFFFFFFFF).sum() > w * h // 64  # the scene is in view
    check(f, cnt, exp, ecnt)


def test_cull_tiles_bounds(oracle):
    """BM_PARAM_CULL_TILES is capped at 2^16 (2^22 rays per region, inside the 32-bit region stride); the cap
    itself is accepted and traces a ragged frame right."""
    ctx = beam.Context(device=0, params={"trace_variant": COMPACT, "trace_sched": 1})
    try:
        for bad in ((1 << 16) + 1, 1 << 26, (1 << 32) - 2):
            with pytest.raises(beam.BeamError) as ei:
                ctx.set_param("cull_tiles", bad)
            assert ei.value.code == beam.ERROR_INVALID_PARAMETER
            assert ctx.get_param("cull_tiles") == -1
        ctx.set_param("cull_tiles", 1 << 16)
        assert ctx.get_param("cull_tiles") == 1 << 16
        run_case(ctx, oracle, "dense", 130, 67, 1 << 16)
    finally:
        ctx.close()
