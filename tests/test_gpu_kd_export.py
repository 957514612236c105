"""Reference mode (BM_OPT_REFERENCE_KD): the kd build itself, leaf by leaf.

bm_scene_kd_export copies out what the march reads — the leaves' path keys, face runs and counts, the
sorted (leaf, face) pairs and the radix tree over the leaf keys — and every case here compares all of it,
by exact integer equality, with the kd oracle's leaves (orc_kd_leaves: key, count and stored faces of every
leaf of the pointer tree) and with a radix tree built top-down in numpy. A frame sees only the leaves a
ray enters and the faces up to its first hit; this sees every leaf, every face in its place, and every
tree node, under each build variant (hand-off depth, walk lanes, workgroup size, box arithmetic, queue
overflow), at the ranked sort digit's 1,024-value edge, at 0, 1 and 2 leaves, and on rebuilt scenes.
"""
import bisect
import contextlib
import functools

import numpy as np
import pytest

from gpu_util import gpu_frame
from raytracercuda_amd import beam, scenes

pytestmark = pytest.mark.gpu

LEAF_BIT = 0x80000000
CAP = 256  # faces a leaf stores (the march tests no more); the counts run on
ONE_LEAF = np.array([[.101, .101, .101], [.102, .101, .101], [.101, .102, .101]], np.float32)
BIG = np.array([[-5, -5, .3], [5, -5, .3], [0, 5, .9]], np.float32)
# a narrow camera just in front of ONE_LEAF: the 0.001-sized triangle covers a good part of the frame
NEAR_CAM, NEAR_EYE = (-0.02, 0.02, -0.02, 0.02, 1.0), (0.1013, 0.1013, 0.05)


def soup(*tris):
    pos = np.concatenate([np.asarray(t, np.float32).reshape(-1, 3) for t in tris])
    nrm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (pos.shape[0], 1))
    return [{"pos": pos, "nrm": nrm, "idx": np.arange(pos.shape[0], dtype=np.uint32)}]


def top_cells(k):
    """One 0.001-sized triangle in each of the first k of the 16 x 16 x 8 cells (3.75 x 3.75 x 7.5) that
    depths 0-10 cut the world into, at the cell's centre plus (0.3, 0.3, 0.3)."""
    c = np.arange(k)
    ctr = np.stack([-30 + 3.75 * (c % 16 + .5), -30 + 3.75 * (c // 16 % 16 + .5), -30 + 7.5 * (c // 256 + .5)], 1) + .3
    tri = np.array([[0, 0, 0], [.001, 0, 0], [0, .001, 0]])
    return soup((ctr[:, None, :] + tri[None]).astype(np.float32))


MESHES = {
    "suzanne": lambda: scenes.load_mesh("suzanne"),
    "f16": lambda: scenes.load_mesh("f16"),
    "bunny": lambda: scenes.load_mesh("bunny"),
    "bunny+big": lambda: scenes.load_mesh("bunny") + soup(BIG),
    "bunny+f16": lambda: scenes.load_mesh("bunny") + scenes.load_mesh("f16"),
    "one_leaf": lambda: soup(ONE_LEAF),
    # the second triangle 0.06 further along z (a leaf is 0.0586 deep there): another leaf, also in view
    "two_leaves": lambda: soup(ONE_LEAF, ONE_LEAF + np.array([.0004, .0004, .06], np.float32)),
    "leaf_cap": lambda: soup(*[ONE_LEAF] * 300),
    "outside": lambda: soup(ONE_LEAF + np.float32(100.0)),
    **{f"cells{k}": functools.partial(top_cells, k) for k in (1, 2, 1024, 1025, 2048)},
}


class OracleTrees:
    """The meshes and the oracle's leaves (keys, counts, stored faces) of each named scene, computed once
    for the module and never changed."""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, name):
        if name not in self.cache:
            meshes = MESHES[name]()
            keys, counts, faces, depth = self.oracle.kd_build(meshes).leaves()
            assert depth == 31 or keys.size == 0
            for a in (keys, counts, faces):
                a.setflags(write=False)
            self.cache[name] = (meshes, (keys, counts, faces))
        return self.cache[name]


@pytest.fixture(scope="module")
def trees(oracle):
    return OracleTrees(oracle)


@pytest.fixture(scope="module")
def kctx():
    c = beam.Context(device=0, reference_kd=True)
    yield c
    c.close()


@contextlib.contextmanager
def built(ctx, meshes, **params):
    """A scene built with the test hooks `params` (bm_context_set_param, read per build; restored after)."""
    for k, v in params.items():
        ctx.set_param(k, v)
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    try:
        st = scene.updateGPUScene(stats=True)
        yield scene, st
    finally:
        scene.destroy()
        del keep
        for k in params:
            ctx.set_param(k, -1)


@functools.lru_cache(maxsize=None)
def _radix_tree(key_bytes):
    """The radix tree over ascending distinct keys, top-down: node [lo, hi] splits at the highest bit in
    which its end keys differ, gamma = the last key with that bit clear; the root is node 0, an internal
    left child [lo, gamma] node gamma, an internal right child [gamma + 1, hi] node gamma + 1, a one-key
    range the leaf reference index | LEAF_BIT."""
    keys = np.frombuffer(key_bytes, np.uint32).tolist()
    n = len(keys)
    lch, rch, first, last = (np.zeros(max(n - 1, 0), np.uint32) for _ in range(4))
    todo = [(0, 0, n - 1)] if n > 1 else []
    while todo:
        i, lo, hi = todo.pop()
        bit = (keys[lo] ^ keys[hi]).bit_length() - 1
        g = bisect.bisect_left(keys, (keys[hi] >> bit) << bit, lo, hi + 1) - 1  # first key with the bit set, less 1
        assert lo <= g < hi
        first[i], last[i] = lo, hi
        lch[i] = g | LEAF_BIT if g == lo else g
        rch[i] = (g + 1) | LEAF_BIT if g + 1 == hi else g + 1
        if g > lo:
            todo.append((g, lo, g))
        if g + 1 < hi:
            todo.append((g + 1, g + 1, hi))
    return lch, rch, first, last


def assert_tree_equal(scene, okd):
    keys, counts, ofaces = okd
    ex = scene.kdExport()
    assert int(scene.kdStats()[0]) == keys.size == ex["leaf_key"].size
    assert np.array_equal(ex["leaf_key"], keys), f"{int((ex['leaf_key'] != keys).sum())} leaf keys differ"
    assert np.array_equal(ex["leaf_count"], counts), f"{int((ex['leaf_count'] != counts).sum())} leaf counts differ"
    c = counts.astype(np.int64)
    start = np.cumsum(c) - c
    assert np.array_equal(ex["leaf_start"], start)
    faces = ex["faces"]
    assert faces.size == int(c.sum())  # M
    # the faces each leaf stores (the first 256 of its run) are the oracle's, in its insertion order
    stored = np.minimum(c, CAP)
    within = np.arange(int(stored.sum())) - np.repeat(np.cumsum(stored) - stored, stored)
    got = faces[np.repeat(start, stored) + within]
    assert np.array_equal(got, ofaces), f"{int((got != ofaces).sum())} of {ofaces.size} stored faces differ"
    # and every run ascends strictly to its end: the order of the ids the cap drops as well
    inside = np.ones(faces.size, bool)
    inside[start[c > 0]] = False
    assert (np.diff(faces.astype(np.int64))[inside[1:]] > 0).all()
    for name, want in zip(("lch", "rch", "first", "last"), _radix_tree(keys.tobytes())):
        assert np.array_equal(ex[name], want), f"{name}: {int((ex[name] != want).sum())} of {want.size} nodes differ"
    return ex


def assert_frame_equal(oracle, ctx, scene, meshes, w, h, cam, eye, hits=True):
    f = gpu_frame(ctx, scene, w, h, cam, eye, scenes.IDENTITY)
    err, rays = oracle.camera_rays(w, h, *cam)
    packed, tri, t = oracle.kd_render(meshes, rays, eye, scenes.IDENTITY)
    assert (tri != 0xFFFFFFFF).any() == hits
    assert np.array_equal(f["tri_id"], tri) and np.array_equal(f["packed"], packed)
    assert np.array_equal(f["t"].view(np.uint32), t.view(np.uint32))
    return tri


@pytest.mark.parametrize("name", ["suzanne", "f16", "bunny", "bunny+big"])
def test_kd_tree_of_meshes(kctx, trees, name):
    """Default parameters. The bunny's 16,742 leaf keys fit the radix-tree kernel's LDS copy; with one large
    triangle more (about 31.7k leaves of its own, far beyond the leaf cache, through childless nodes) there
    are more than 32,768 and it searches the keys in global memory. That triangle reaches more nodes at the
    hand-off depth than a workgroup's queue holds: the ones walked on mark the top-bit map as well, so the
    sort keeps its ranked digit."""
    meshes, okd = trees(name)
    if name == "bunny":
        assert 2 <= okd[0].size <= 32768
    if name == "bunny+big":
        assert okd[0].size > 32768
    with built(kctx, meshes) as (scene, st):
        assert st["sort_path"] == beam.SORT_KD_RANKED
        assert_tree_equal(scene, okd)


@pytest.mark.parametrize("split", [0, 1, 8, 10, 11, 12, 25, 30])
def test_kd_tree_at_every_hand_off_depth(kctx, trees, split):
    """BM_PARAM_KD_SPLIT: 0 walks each triangle in one lane (k_kd_descend); below 11 the queued nodes
    cannot mark the top 11 path bits, so the pair sort runs its four plain passes (BM_SORT_LSD) — with a
    map nobody filled it once ran three and left the pairs ordered by bits 0-19 only; from 11 up the
    ranked digit (BM_SORT_KD_RANKED)."""
    meshes, okd = trees("suzanne")
    with built(kctx, meshes, kd_split=split) as (scene, st):
        assert_tree_equal(scene, okd)
        assert st["sort_path"] == (beam.SORT_LSD if split <= 10 else beam.SORT_KD_RANKED), st["sort_path"]


def test_kd_frame_with_shallow_hand_off(kctx, trees, oracle):
    meshes, okd = trees("bunny")
    with built(kctx, meshes, kd_split=8) as (scene, st):
        assert_frame_equal(oracle, kctx, scene, meshes, 128, 96, scenes.RAYS_1080, scenes.BUNNY_EYE)
        assert_tree_equal(scene, okd)
        assert st["sort_path"] == beam.SORT_LSD, st["sort_path"]


WALKS = [dict(kd_pair=p, kd_tb=tb, kd_grid=g) for p in (0, 1) for tb in (64, 256) for g in (0, 1)]
# 256-lane workgroups of one-lane walks with queues too small for the work: the walk-on paths
WALKS += [dict(kd_pair=0, kd_tb=256, kd_grid=g, kd_lq_cap=3, kd_queue_cap=40) for g in (0, 1)]


@pytest.mark.parametrize("split", [8, None])
@pytest.mark.parametrize("walk", WALKS, ids=lambda w: "-".join(f"{k[3:]}{v}" for k, v in w.items()))
def test_kd_tree_under_every_walk(kctx, trees, walk, split):
    """k_kd_top / k_kd_sub <EMIT, PAIR, TB, GRID>: one or two lanes per walk, 64-lane workgroups (walks
    sharing work) or 256-lane ones (each on its own stack), node boxes by the closed form or the halving
    recurrence, at a shallow hand-off depth and the default one."""
    meshes, okd = trees("suzanne")
    params = dict(walk) if split is None else dict(walk, kd_split=split)
    with built(kctx, meshes, **params) as (scene, st):
        assert_tree_equal(scene, okd)


@pytest.mark.parametrize("k", [1, 2, 1024, 1025, 2048])
def test_kd_tree_at_the_ranked_digit_edge(kctx, trees, k):
    """k values of the leaf paths' top 11 bits: the ranked digit holds up to 1,024, one more takes the
    four plain passes."""
    meshes, okd = trees(f"cells{k}")
    assert np.unique(okd[0] >> 20).size == k
    with built(kctx, meshes) as (scene, st):
        assert st["sort_path"] == (beam.SORT_KD_RANKED if k <= 1024 else beam.SORT_LSD), st
        assert_tree_equal(scene, okd)


def test_kd_leaf_beyond_the_cap(kctx, trees):
    meshes, okd = trees("leaf_cap")
    assert okd[1].tolist() == [300] and okd[2].tolist() == list(range(256))  # 44 dropped
    with built(kctx, meshes) as (scene, st):
        ex = assert_tree_equal(scene, okd)
        assert ex["leaf_count"].tolist() == [300] and ex["faces"].tolist() == list(range(300))
        assert scene.kdStats().tolist() == [1, 256, 44, 300]


@pytest.mark.parametrize("name,leaves", [("one_leaf", 1), ("two_leaves", 2), ("outside", 0)])
def test_kd_tree_and_frame_of_degenerate_sizes(kctx, trees, oracle, name, leaves):
    """One leaf (no radix tree, the march starts at the leaf), two (one internal node), and none (a
    triangle outside the world: no pairs, empty arrays, every pixel a miss)."""
    meshes, okd = trees(name)
    assert okd[0].size == leaves
    with built(kctx, meshes) as (scene, st):
        ex = assert_tree_equal(scene, okd)
        assert ex["faces"].size == leaves and ex["lch"].size == max(leaves - 1, 0)
        tri = assert_frame_equal(oracle, kctx, scene, meshes, 64, 48, NEAR_CAM, NEAR_EYE, hits=leaves > 0)
        assert np.unique(tri[tri != 0xFFFFFFFF]).size == leaves  # every leaf's triangle is seen


def test_kd_rebuilds_on_reused_buffers(kctx, trees):
    """One scene rebuilt with its buffers, scan epochs, sort metadata, top-bit map and queue reused:
    twice the same meshes, then fewer, then all again."""
    both, okd_both = trees("bunny+f16")
    bunny, okd_bunny = trees("bunny")
    scene = beam.IScene.create(kctx)
    keep = beam.upload_meshes(kctx, scene, both)
    try:
        scene.updateGPUScene()
        ex1 = assert_tree_equal(scene, okd_both)
        scene.updateGPUScene()
        ex2 = assert_tree_equal(scene, okd_both)
        assert all(np.array_equal(ex1[k], ex2[k]) for k in ex1)
        f16 = keep[len(bunny):]
        for m in f16:
            scene.removeMesh(m)
        scene.updateGPUScene()
        assert_tree_equal(scene, okd_bunny)
        for m in f16:
            scene.addMesh(m)
        scene.updateGPUScene()
        assert_tree_equal(scene, okd_both)
    finally:
        scene.destroy()
        del keep


def test_kd_export_needs_a_reference_mode_build(kctx, ctx, trees):
    meshes, _ = trees("one_leaf")
    scene = beam.IScene.create(kctx)
    keep = beam.upload_meshes(kctx, scene, meshes)
    with pytest.raises(beam.BeamError) as e:
        scene.kdExport()
    assert e.value.code == beam.ERROR_NOT_BUILT
    scene.destroy()
    with built(ctx, meshes) as (bvh, st):
        m = np.zeros(1, np.uint64)
        r = ctx.lib.bm_scene_kd_export(bvh.h, m.ctypes.data_as(beam.C.POINTER(beam.C.c_uint64)), *([None] * 8))
        assert r == beam.ERROR_INVALID_PARAMETER
    del keep
