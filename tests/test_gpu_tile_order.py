"""The quad kernel's cost-ordered tile schedule (k_trace_quad, sched 2) under injected cost tables.

Each workgroup sorts its share of the frame's 4x4 tiles by the tick counts the previous trace of the render
target recorded (tile_cost) and hands them out longest first. A frame may not depend on that order: the sort,
the XCD-aware tile map and the ticket loop must hand out every tile of the share exactly once for any table.
A green run only ever sees the costs the GPU happened to record, so bm_rt_debug_tile_costs injects the tables
timing never produces: zeros, ties, saturated values (>= 2^18 per tile, the run clamp), one heavy tile, runs
of 8 with equal sums, and a marker table (every word >= 2^31, which no tick count reaches).

Every case injects a table, runs the counting trace, injects again (a trace rewrites the table) and runs the
plain trace. Ids, packed colours and t are bit-equal to the oracle's (no tile dropped) and the node, triangle
and hit counters equal the oracle's (no tile traced twice). After the marker table's plain trace the table is
read back: with the schedule on every word below ntiles was rewritten and the 64 guard words after it were
not; with it off (lpt_share_fits false, a grid without the XCD map, BVH2) nothing was touched.

The grids are set with trace_grid: 8 at 960 tiles (share 120 + 8 = LPT_MAX, the last that fits) and 961 (one
past), 24/56/72 (xblocks % 8 != 0: the per-tile keys, which no default grid of the product device reaches),
64 (run keys, last run clipped by the frame), 128 (most shares empty), the default, and 1/3/12/20 (no XCD map).

Measured on an MI355X: the file takes 0.9 s of wall time (22 tests).
"""
import numpy as np
import pytest

from raytracercuda_amd import beam, scenes
from test_gpu_variants import check, expect

pytestmark = pytest.mark.gpu

QUAD = 10
LPT_MAX = 128    # bm_trace_quad.h
GUARD = 64
EYE = (0.1, 0.05, -3.0)
LIGHT = (0.0, 10.0, -10.0)
CAM = scenes.RAYS_SQUARE


def scene_meshes():
    """40 random triangles (test_variant_ragged_frames' scene)."""
    rng = np.random.default_rng(4021)
    n = 40
    return [{"pos": rng.uniform(-1, 1, size=(3 * n, 3)).astype(np.float32),
             "nrm": rng.normal(size=(3 * n, 3)).astype(np.float32), "idx": np.arange(3 * n, dtype=np.uint32)}]


MESHES = scene_meshes()
_expected = {}


def expected(oracle, w, h, eye=EYE, width=4, light=None):
    """The oracle's frame and counters, computed once per view and shared (never modified)."""
    key = (w, h, tuple(eye), width, light)
    if key not in _expected:
        _expected[key] = expect(oracle, MESHES, w, h, CAM, eye, scenes.IDENTITY, width=width, light=light)
    return _expected[key]


def quad_tiles(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)


def share_fits(ntiles, blocks):
    """lpt_share_fits (bm_trace_quad.h): whether k_trace_quad orders a frame of ntiles over this grid by cost."""
    return blocks >= 8 and blocks % 8 == 0 and (ntiles + blocks - 1) // blocks + 8 <= LPT_MAX


def cost_tables(ntiles):
    """name -> uint32[ntiles + GUARD]: the tables of the issue, each followed by guard words (>= 2^31)."""
    rng = np.random.default_rng(ntiles)
    i = np.arange(ntiles, dtype=np.uint64)
    t = {"zeros": np.zeros(ntiles, np.uint64),
         "equal": np.full(ntiles, 777, np.uint64),
         "ascending": i + 1,
         "descending": ntiles - i,
         "random18": rng.integers(0, 1 << 18, ntiles, dtype=np.uint64),
         "random32": rng.integers(0, 1 << 32, ntiles, dtype=np.uint64),
         "heavy_first": np.where(i == 0, 1 << 17, 3).astype(np.uint64),
         "heavy_last": np.where(i == ntiles - 1, 1 << 17, 3).astype(np.uint64),
         # run r holds 1 + 1000 * ((j + r) % 8): every whole run sums alike, no two neighbours hold the same members
         "equal_runs": 1 + 1000 * ((i % 8 + i // 8) % 8),
         "marker": (1 << 31) | ((i * 2654435761 + 12345) & 0x7FFFFFFF)}
    r32 = t["random32"]
    for k, v in enumerate((0xFFFFFFFF, 1 << 18, 1 << 22, 0, (1 << 18) - 1, (1 << 22) - 1, 0xFFFFFFFF, 1 << 31)):
        r32[(k * 7) % ntiles] = v  # saturated per tile (>= 2^18), per key (>= 2^22) and the largest word, wherever
    r32[8 % ntiles:16] = 0xFFFFFFFF  # a whole run saturated
    guard = (0xA5A50000 + np.arange(GUARD)).astype(np.uint32)
    return {k: np.concatenate([v.astype(np.uint32), guard]) for k, v in t.items()}


class Rig:
    """One scene, camera and render target of w x h on a context."""

    def __init__(self, ctx, w, h):
        self.ctx, self.w, self.h = ctx, w, h
        self.scene = beam.IScene.create(ctx)
        self.keep = beam.upload_meshes(ctx, self.scene, MESHES)
        self.scene.updateGPUScene()
        self.cam = beam.ICamera.create(ctx)
        assert self.cam.setInitialRays(w, h, *CAM) == 0
        self.rt = beam.IRenderTarget.createOffscreen(ctx, w, h)

    def render(self, table=None, eye=EYE, light=None):
        """test_gpu_variants.render with the table injected before each of its two traces."""
        c, rt, sc = self.cam, self.rt, self.scene
        if table is not None:
            rt.debugTileCosts(set=table)
        if light is None:
            cnt = c.traceCounters(eye, scenes.IDENTITY, sc, rt)
        else:
            cnt = c.traceShadowCounters(eye, scenes.IDENTITY, sc, rt, light)
        if table is not None:
            rt.debugTileCosts(set=table)
        if light is None:
            assert c.trace(eye, scenes.IDENTITY, sc, rt) == 0
        else:
            assert c.traceShadow(eye, scenes.IDENTITY, sc, rt, light) == 0
        f = {k: v.reshape(-1) for k, v in rt.read().items()}
        if light is not None:
            f["shadow"] = rt.readShadow().reshape(-1)
        return f, cnt

    def close(self):
        self.rt.destroy()
        self.cam.destroy()
        self.scene.destroy()
        self.keep = None


@pytest.fixture
def make_ctx():
    made = []

    def make(grid=None, default=False, **kw):
        params = {} if default else {"trace_variant": QUAD, "trace_sched": 2}
        if grid is not None:
            params["trace_grid"] = grid
        c = beam.Context(device=0, params=params, **kw)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


def default_grid_has_xcd_map(rig):
    """The default persistent grid is a whole number of workgroups per CU, so a multiple of 8 when the CU count
    is. bm_camera_trace_profile, asked for its buffer size only, reports the waves of 8 workgroups per CU."""
    n = beam.C.c_uint32(0)
    rig.ctx.lib.bm_camera_trace_profile(rig.cam.h, None, None, rig.scene.h, rig.rt.h, None, 0, beam.C.byref(n))
    assert n.value and n.value % 32 == 0
    return (n.value // 32) % 8 == 0


def run_tables(rig, oracle, on, light=None, width=4):
    """Every table through the rig; collects each failure and names them all."""
    ntiles = quad_tiles(rig.w, rig.h)
    exp, ecnt = expected(oracle, rig.w, rig.h, width=width, light=light)
    bad = []
    for name, table in cost_tables(ntiles).items():
        f, cnt = rig.render(table, light=light)
        try:
            check(f, cnt, exp, ecnt)
        except AssertionError as e:
            bad.append(f"{name}: {e}")
        if name != "marker":
            continue
        # the marker table after the non-counting full-frame trace
        back = rig.rt.debugTileCosts(get=ntiles + GUARD)
        if on:
            same = int((back[:ntiles] == table[:ntiles]).sum())
            if same:
                bad.append(f"marker: {same} of {ntiles} table words were not rewritten")
            if not np.array_equal(back[ntiles:], table[ntiles:]):
                bad.append("marker: guard words after ntiles were overwritten")
        elif not np.array_equal(back, table):
            bad.append(f"marker: schedule off, yet {int((back != table).sum())} table words changed")
    assert not bad, "\n".join(bad)


GRID_ROWS = [(8, 160, 96), (8, 124, 124), (8, 37, 23), (24, 150, 91), (56, 150, 91), (72, 150, 91), (64, 150, 91),
             (64, 256, 256), (128, 37, 23), (None, 150, 91), (1, 150, 91), (3, 150, 91), (12, 150, 91), (20, 150, 91)]


def test_share_boundary_is_where_the_issue_puts_it():
    """The rows of GRID_ROWS reach what they are there for (host arithmetic only)."""
    assert quad_tiles(160, 96) == 960 and share_fits(960, 8) and (960 + 7) // 8 + 8 == LPT_MAX
    assert quad_tiles(124, 124) == 961 and not share_fits(961, 8)
    assert quad_tiles(37, 23) == 60 and quad_tiles(150, 91) == 874 and quad_tiles(256, 256) == 4096
    for g in (24, 56, 72):  # per-tile keys: xblocks % 8 != 0
        assert share_fits(874, g) and (g // 8) % 8 != 0
    assert share_fits(874, 64) and share_fits(4096, 64) and (64 // 8) % 8 == 0 and 874 % 8 != 0
    assert share_fits(60, 128)
    for g in (1, 3, 12, 20):
        assert not share_fits(874, g)


@pytest.mark.parametrize("grid,w,h", GRID_ROWS, ids=[f"grid{g}-{w}x{h}" for g, w, h in GRID_ROWS])
def test_injected_cost_tables(make_ctx, oracle, grid, w, h):
    ctx = make_ctx(grid) if grid is not None else make_ctx(default=True)
    if grid is not None:
        on = share_fits(quad_tiles(w, h), grid)
    else:
        assert ctx.get_param("trace_grid") == -1 and ctx.get_param("trace_sched") == -1
    rig = Rig(ctx, w, h)
    try:
        if grid is None:
            on = default_grid_has_xcd_map(rig)
        run_tables(rig, oracle, on)
        assert rig.rt.traceKind() == "quads"
    finally:
        rig.close()


def test_injected_cost_tables_fused_shadow(make_ctx, oracle):
    """traceShadow and its counters under every table, against the oracle's shadow plane (per-tile keys)."""
    rig = Rig(make_ctx(24), 150, 91)
    try:
        run_tables(rig, oracle, True, light=LIGHT)
    finally:
        rig.close()


def test_bvh2_leaves_the_table_alone(make_ctx, oracle):
    """A BVH2 scene takes the single-lane kernel under the same parameters: right frame, table untouched."""
    rig = Rig(make_ctx(64, bvh_width=2), 150, 91)
    try:
        run_tables(rig, oracle, False, width=2)
        assert rig.rt.traceKind() == "lanes"
    finally:
        rig.close()


@pytest.mark.parametrize("width", [4, 2])
def test_empty_scene_counts_the_root_record(make_ctx, oracle, width):
    """No triangles: every pixel a miss, and the counting trace reports the one all-empty root record per ray
    that the oracle visits (the quad kernel and, for BVH2, the single-lane kernel). Exposed by the empty scene
    of tests/test_gpu_ray_queue.py, where k_cull counted nothing."""
    ctx = make_ctx(64, bvh_width=width) if width == 2 else make_ctx(64)
    w, h = 37, 23
    scene = beam.IScene.create(ctx)
    scene.updateGPUScene()
    cam = beam.ICamera.create(ctx)
    assert cam.setInitialRays(w, h, *CAM) == 0
    rt = beam.IRenderTarget.createOffscreen(ctx, w, h)
    cnt = cam.traceCounters(EYE, scenes.IDENTITY, scene, rt)
    assert cam.trace(EYE, scenes.IDENTITY, scene, rt) == 0
    f = {k: v.reshape(-1) for k, v in rt.read().items()}
    rt.destroy()
    cam.destroy()
    scene.destroy()
    exp, ecnt = expect(oracle, [], w, h, CAM, EYE, scenes.IDENTITY, width=width)
    assert list(ecnt) == [w * h, 0, 0]
    check(f, cnt, exp, ecnt)


def test_stale_table_from_another_band_layout(make_ctx, oracle):
    """A random table sized for the full frame, then band traces (16 rows, 3 ranks) into the same target:
    the bands' tile numbering is not the table's. Each rank's rows equal the oracle's full frame."""
    w, h, bh, n = 150, 91, 16, 3
    rig = Rig(make_ctx(64), w, h)
    try:
        exp, _ = expected(oracle, w, h)
        table = cost_tables(quad_tiles(w, h))["random32"]
        bands = (h + bh - 1) // bh
        for r in range(n):
            rig.rt.debugTileCosts(set=table)
            assert rig.cam.traceBands(EYE, scenes.IDENTITY, rig.scene, rig.rt, bh, n, r) == 0
            part = rig.rt.read()
            for i, b in enumerate(b for b in range(bands) if b % n == r):
                rows = slice(b * bh, min((b + 1) * bh, h))
                k = rows.stop - rows.start
                for plane in ("packed", "tri_id", "t"):
                    got = part[plane][i * bh:i * bh + k].view(np.uint32)
                    want = exp[plane].reshape(h, w)[rows].view(np.uint32)
                    assert np.array_equal(got, want), f"rank {r} band {b} {plane}"
    finally:
        rig.close()


def test_consecutive_frames_on_real_timings(make_ctx, oracle):
    """No injection: three frames from moving eyes into one target, each ordered by the previous frame's
    recorded times, each equal to the oracle's."""
    rig = Rig(make_ctx(64), 150, 91)
    try:
        for eye in ((0.1, 0.05, -3.0), (0.3, -0.1, -2.8), (-0.4, 0.2, -3.3)):
            f, cnt = rig.render(None, eye=eye)
            check(f, cnt, *expected(oracle, 150, 91, eye=eye))
    finally:
        rig.close()


def test_debug_tile_costs_refusals(make_ctx):
    ctx = make_ctx(64)
    rt = beam.IRenderTarget.createOffscreen(ctx, 16, 16)
    word = np.zeros(1, np.uint32)
    p = word.ctypes.data_as(beam.C.POINTER(beam.C.c_uint32))
    assert ctx.lib.bm_rt_debug_tile_costs(rt.h, 0, p, None) == beam.ERROR_INVALID_PARAMETER
    assert ctx.lib.bm_rt_debug_tile_costs(rt.h, 1, None, None) == beam.ERROR_INVALID_PARAMETER
    assert ctx.lib.bm_rt_debug_tile_costs(None, 1, p, None) == beam.ERROR_INVALID_PARAMETER
    rt.debugTileCosts(set=[5, 6, 7])
    assert list(rt.debugTileCosts(get=3)) == [5, 6, 7]
    rt.destroy()
    multi = make_ctx(devices=[0, 0])  # one GPU rehearsing two
    mrt = beam.IRenderTarget.createOffscreen(multi, 16, 16)
    assert multi.lib.bm_rt_debug_tile_costs(mrt.h, 1, p, None) == beam.ERROR_INVALID_PARAMETER
    mrt.destroy()
