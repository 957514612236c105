"""The deep-stack fixture (tests/deep_scenes.py) and the oracle on it, without a GPU.

tests/test_gpu_stack_overflow.py compares every ray kernel with the oracle on frames and batches whose
rays outgrow the kernels' LDS stacks. This file checks, for each of those frames and batches, that
  * the oracle's traversal (which pushes in the GPU's order: the traversal counters match) really holds
    more than 24 entries for at least a quarter of the rays, and never more than MAX_STACK = 96;
  * the frame is no degenerate one (hits and misses, several triangles, lit and shadowed pixels);
  * the oracle's BVH answers equal the exhaustive ones, so the GPU is compared with something that was
    itself checked.
The per-ray depth comes from the oracle's orc_set_ray_depth hook (OrcBVH.render/shadow depth=...).

The hit-fraction and shadow-fraction bounds hold for the "axis" and "mixed" views. The "diag" view is
kept for what it is there for (a quarter of its rays deep, the rest shallow, in the same waves): only 2
to 3 % of its rays hit and all of those are shadowed, so for it the test asserts depth, ceiling,
distinct triangles, the shadow rays' depth and the exhaustive answers, not those two fractions.

test_depth_of_the_older_parity_views prints, and does not assert, how deep the views of the older GPU
parity tests go: whether the suite reached the overflow side before this fixture existed.
"""
import threading

import numpy as np
import pytest

import deep_scenes as ds
from golden_io import manifest
from raytracercuda_amd import scenes

WIDTHS = (4, 2)
FRAMES = [(name, width, view, size) for name, _, _ in ds.SCENES for width in WIDTHS for view in ds.VIEWS
          for size in ds.SIZES]


def frame_id(c):
    return f"{c[0]}-w{c[1]}-{c[2]}-{c[3][0]}x{c[3][1]}"


def assert_depth(depth, what):
    share = float((depth > ds.QUAD_LDS).mean())
    assert share >= 0.25, f"{what}: only {share:.3f} of the rays hold more than {ds.QUAD_LDS} entries"
    assert int(depth.max()) <= ds.MAX_STACK, f"{what}: deepest stack {int(depth.max())} > {ds.MAX_STACK}"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", FRAMES, ids=frame_id)
def test_frames_are_deep_and_the_oracle_is_right_on_them(oracle, case):
    name, width, view, size = case
    with_light = size == ds.SIZES[0]  # the shadow tests trace the 64x48 frames
    e = ds.expected(oracle, name, width, view, size, light=ds.LIGHT if with_light else None)
    s = e.stats
    print(f"{frame_id(case)}: {ds.fmt(s)}")
    assert_depth(e.depth, "primary rays")
    assert s["distinct"] >= 8, s
    if view != "diag":
        assert 0.10 <= s["hit"] <= 0.90, s
    else:
        assert 0.0 < s["hit"] < 1.0 and 0.25 <= s[f">{ds.QUAD_LDS}"] <= 0.75, s  # deep and shallow rays mixed
    meshes, _ = ds.oracle_bvh(oracle, name, width)
    packed, tri, t = oracle.brute_render(meshes, e.rays, e.eye, e.orient)
    assert np.array_equal(e.frame["tri_id"], tri)
    assert np.array_equal(e.frame["packed"], packed)
    assert np.array_equal(bits(e.frame["t"]), bits(t))
    if with_light:
        hit = tri != ds.MISS
        assert np.all(e.sdepth[~hit] == 0)  # no shadow ray is cast there
        assert s["shadow>24"] >= 0.25 and s["shadow_deepest"] <= ds.MAX_STACK, s
        if view != "diag":
            assert 0.10 <= s["shadowed"] <= 0.90, s
        assert np.array_equal(e.frame["shadow"], oracle.brute_shadow(meshes, e.rays, e.eye, e.orient, ds.LIGHT, tri, t))


@pytest.mark.parametrize("view", [v for v in ds.FLIGHT_VIEWS if v not in ds.VIEWS])
def test_frames_in_flight_are_deep(oracle, view):
    e = ds.expected(oracle, "deep", 4, view, ds.SIZES[0])
    print(f"deep-w4-{view}: {ds.fmt(e.stats)}")
    assert_depth(e.depth, "primary rays")
    assert 0.10 <= e.stats["hit"] <= 0.90 and e.stats["distinct"] >= 8, e.stats
    meshes, _ = ds.oracle_bvh(oracle, "deep", 4)
    _, tri, t = oracle.brute_render(meshes, e.rays, e.eye, e.orient)
    assert np.array_equal(e.frame["tri_id"], tri) and np.array_equal(bits(e.frame["t"]), bits(t))
    first = ds.expected(oracle, "deep", 4, "axis", ds.SIZES[0])
    assert not np.array_equal(e.frame["tri_id"], first.frame["tri_id"])  # three different frames


@pytest.mark.parametrize("name", ds.QUERY_SCENES)
def test_query_batches_are_deep_and_the_oracle_is_right_on_them(oracle, name):
    meshes, obvh = ds.oracle_bvh(oracle, name, 4)
    q = ds.query_expected(oracle, name)
    s = ds.query_stats(q.depth, q.exp["tri_id"] != ds.MISS)
    print(f"{name}: closest-hit batch of {q.o.shape[0]} rays: {ds.fmt(s)}")
    assert q.o.shape[0] % 16 != 0
    assert_depth(q.depth, "closest-hit batch")
    assert 0.10 <= s["hit"] <= 0.90 and np.unique(q.exp["tri_id"]).size >= 9, s
    for g in range(ds.QUERY_ORIGINS.shape[0]):  # rays g, g + 4, ... share origin g
        sel = slice(g, None, ds.QUERY_ORIGINS.shape[0])
        assert np.all(q.o[sel] == ds.QUERY_ORIGINS[g])
        _, tri, t = oracle.brute_render(meshes, q.d[sel], ds.QUERY_ORIGINS[g], ds.IDENTITY)
        assert np.array_equal(q.exp["tri_id"][sel], tri) and np.array_equal(bits(q.exp["t"][sel]), bits(t))
        sg = ds.query_stats(q.depth[sel], tri != ds.MISS)
        print(f"  origin {tuple(ds.QUERY_ORIGINS[g])}: {ds.fmt(sg)}")
        assert sg[">24"] >= 0.25 and 0.10 <= sg["hit"] <= 0.90, sg
    # interleaved with shallow rays: every other ray's stack stays empty
    assert np.all(q.mix_depth[1::2] == 0) and np.array_equal(q.mix_depth[0::2], q.depth[:q.mix_depth.size // 2])
    assert np.all(q.mix_exp["tri_id"][1::2] == ds.MISS)
    s = ds.query_stats(q.seg_depth, q.occ)
    print(f"{name}: any-hit batch of {q.a.shape[0]} segments: {ds.fmt(s)}")
    assert_depth(q.seg_depth, "any-hit batch")
    assert 0.10 <= s["hit"] <= 0.90, s
    assert np.all(q.a + q.seg_d == q.b)  # the end point reproduces d exactly
    zero_tri, zero_t = np.zeros(1, np.uint32), np.zeros(1, np.float32)
    brute = np.array([oracle.brute_shadow(meshes, ds.ONE_RAY, q.a[i], ds.IDENTITY, q.b[i], zero_tri, zero_t)[0]
                      for i in range(q.a.shape[0])], np.uint8)
    assert np.array_equal(q.occ, brute)


def test_depth_hook_is_per_thread_and_leaves_the_answers_alone(oracle):
    """Two threads trace different frames at once, each with its own depth array (bench.py's CPU baseline
    calls the trace from several threads); a call without the hook writes nothing."""
    _, obvh = ds.oracle_bvh(oracle, "deep", 4)
    deep = ds.expected(oracle, "deep", 4, "axis", ds.SIZES[0])
    mixed = ds.expected(oracle, "deep", 4, "diag", ds.SIZES[0])
    out = {}

    def work(key, e):
        for _ in range(4):
            d = np.zeros(e.rays.shape[0], np.uint32)
            _, tri, _ = obvh.render(e.rays, e.eye, e.orient, depth=d)
            out[key] = (d, tri)
            plain = obvh.render(e.rays, e.eye, e.orient)  # no hook: same frame
            assert np.array_equal(plain[1], tri)

    threads = [threading.Thread(target=work, args=(k, e)) for k, e in (("deep", deep), ("mixed", mixed))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k, e in (("deep", deep), ("mixed", mixed)):
        assert np.array_equal(out[k][0], e.depth) and np.array_equal(out[k][1], e.frame["tri_id"])
    with pytest.raises(ValueError):
        obvh.render(deep.rays, deep.eye, deep.orient, depth=np.zeros(3, np.uint32))
    # a range of pixels: only [begin, end) is written
    d = np.full(deep.rays.shape[0], 777, np.uint32)
    obvh.render(deep.rays, deep.eye, deep.orient, begin=100, end=200, depth=d)
    assert np.all(d[:100] == 777) and np.all(d[200:] == 777) and np.array_equal(d[100:200], deep.depth[100:200])


def test_depth_of_the_older_parity_views(oracle):
    """Printed, not asserted: the deepest stack of the views the older GPU parity tests trace."""
    from test_gpu_rays import make_batch
    m = manifest()["views"]["bunny_256"]
    views = [("bunny_256", "bunny", 4, m["w"], m["h"], tuple(m["rays"]), tuple(m["eye"])),
             ("bunny 480x270", "bunny", 4, 480, 270, scenes.RAYS_1080, scenes.BUNNY_EYE),
             ("suzanne 480x270", "suzanne", 1, 480, 270, scenes.RAYS_1080, (0.0, 0.0, -3.0)),
             ("f16 480x270", "f16", 16, 480, 270, scenes.RAYS_1080, (0.0, 0.0, -3.0))]
    for label, mesh, leaf, w, h, cam, eye in views:
        meshes = scenes.load_mesh(mesh)
        for width in WIDTHS:
            err, rays = oracle.camera_rays(w, h, *cam)
            assert err == 0
            depth = np.zeros(w * h, np.uint32)
            oracle.bvh_build(meshes, leaf, width).render(rays, eye, scenes.IDENTITY, depth=depth)
            print(f"{label}, leaf {leaf}, BVH{width}: deepest stack {int(depth.max())}, rays beyond 8/12/16/24: "
                  + "/".join(str(int((depth > k).sum())) for k in (8, 12, 16, 24)))
    for mesh in ("suzanne", "bunny"):
        meshes = scenes.load_mesh(mesh)
        o, d = make_batch(meshes)
        _, _, depth = ds.closest_expected(oracle, oracle.bvh_build(meshes, 4, 4), meshes, o, d)
        print(f"{mesh}, the {o.shape[0]}-ray query batch, leaf 4, BVH4: deepest stack {int(depth.max())}, rays beyond "
              "8/12/16/24: " + "/".join(str(int((depth > k).sum())) for k in (8, 12, 16, 24)))
