"""The oracle's build at every leaf size 1..16 and every width, without a GPU.

tests/test_gpu_leaf_sizes.py compares the GPU build with the oracle's at every leaf size and runs every batch
query on scenes built with leaves of up to 16 triangles. This file checks what those comparisons rest on:
  * the oracle's own build is a partition at every leaf size and width: every triangle in exactly one reachable
    leaf, no leaf above the leaf size, each leaf's box around its triangles' vertices;
  * on the F-16 every leaf count 1..L occurs at width 4, so a build at L evaluates leaves of every group shape
    (the query kernels take a leaf four triangles at a time: 1..3 lanes, full groups, full groups plus a tail);
  * the oracle's closest hits equal its exhaustive test off the default leaf size;
  * the pile of tests/leaf_scenes.py fills leaves of its own: at leaf size 16, at least two leaves of nine or
    more triangles hold pile triangles only.
"""
import numpy as np
import pytest

import leaf_scenes as ls
from raytracercuda_amd import scenes
from test_multihit_abi import make_batch

MISS = 0xFFFFFFFF
WIDTHS = (2, 4, 8)
GROUPS, PER = 8, 64  # one batch of 512 rays


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("leaf", ls.LEAF_SIZES)
def test_every_leaf_size_builds_a_partition(oracle, leaf, width):
    meshes = ls.f16_meshes()
    rec, tris, keys, perm = oracle.bvh_build(meshes, leaf, width).export()
    ntri = tris.shape[0]
    assert ntri == 4056 and rec.shape[1] == {2: 16, 4: 32, 8: 64}[width]
    lv = ls.leaves(rec, tris)
    seen = np.zeros(ntri, np.int64)
    hist = np.zeros(17, np.int64)
    for first, cnt, lo, hi, ids in lv:
        assert 1 <= cnt <= leaf and first + cnt <= ntri, (first, cnt)
        seen[first:first + cnt] += 1
        hist[cnt] += 1
        pts = ls.leaf_corners(tris, first, cnt)
        assert (pts >= lo).all() and (pts <= hi).all(), (first, cnt)
    assert (seen == 1).all(), f"{int((seen != 1).sum())} triangle records lie in no leaf or in several"
    assert np.array_equal(np.sort(tris[:, 3]), np.arange(ntri, dtype=np.uint32))  # and the records hold every id once
    print(f"f16, leaf size {leaf}, BVH{width}: {len(lv)} leaves, by count {hist[1:leaf + 1].tolist()}")
    if width == 4:
        assert (hist[1:leaf + 1] > 0).all(), f"no leaf of {np.flatnonzero(hist[1:leaf + 1] == 0) + 1} triangles"
    assert hist[leaf + 1:].sum() == 0


def test_the_width_does_not_change_the_leaves(oracle):
    """The collapse into wider nodes moves no triangle: BVH2, BVH4 and BVH8 hold the same leaves."""
    meshes = ls.scene_meshes()
    for leaf in (1, 3, 7, 13, 16):
        runs = []
        for width in WIDTHS:
            rec, tris, _, _ = oracle.bvh_build(meshes, leaf, width).export()
            runs.append(sorted((first, cnt) for first, cnt, _, _, _ in ls.leaves(rec, tris)))
        assert runs[0] == runs[1] == runs[2], leaf


def ray_batch(meshes):
    """512 rays in 8 groups of 64 that share an origin: seven eyes around the scene (make_batch's scheme) and one
    below the pile, its rays aimed through the pile's triangles."""
    o, d = make_batch(meshes, groups=GROUPS, per=PER, seed=19)
    rng = np.random.default_rng(23)
    eye = np.float32([ls.PILE_AXIS[0], ls.PILE_AXIS[1], ls.PILE_AT[2] - 1.0])
    top = np.float32([ls.PILE_AT[0], ls.PILE_AT[1], ls.PILE_AT[2] + ls.PILE_N * ls.PILE_STEP])
    targets = top + np.float32(rng.uniform(0.0, 0.25, (PER, 3)) * [1, 1, 0])
    o[-PER:] = eye
    d[-PER:] = (targets - eye) + np.float32(0.0)
    return o, d


@pytest.mark.parametrize("leaf", [3, 7, 13, 16])
def test_closest_hits_equal_the_exhaustive_test(oracle, leaf):
    meshes = ls.scene_meshes()
    o, d = ray_batch(meshes)
    assert o.shape[0] == 512
    obvh = oracle.bvh_build(meshes, leaf, 4)
    hits, on_pile = 0, 0
    pile = ls.pile_ids()
    for g in range(0, o.shape[0], PER):
        assert np.all(o[g:g + PER] == o[g])
        packed, tri, t = obvh.render(d[g:g + PER], o[g], scenes.IDENTITY)
        bp, btri, bt = oracle.brute_render(meshes, d[g:g + PER], o[g], scenes.IDENTITY)
        assert np.array_equal(tri, btri) and np.array_equal(bits(t), bits(bt)) and np.array_equal(packed, bp)
        hits += int((tri != MISS).sum())
        on_pile += int(np.isin(tri, pile).sum())
    assert 0.1 * 512 <= hits <= 0.9 * 512, hits
    assert on_pile >= 16, on_pile  # the lowest pile triangle, from below: the first of a leaf of several


def test_the_pile_fills_leaves_of_its_own(oracle):
    meshes = ls.scene_meshes()
    pile = ls.pile_ids()
    assert pile.size == ls.PILE_N == 40 and pile[0] == 4056
    for leaf in ls.QUERY_LEAF_SIZES:
        rec, tris, _, _ = oracle.bvh_build(meshes, leaf, 4).export()
        lv = ls.leaves(rec, tris)
        hist = np.bincount([x[1] for x in lv], minlength=17)
        own = sorted(x[1] for x in lv if np.isin(x[4], pile).all())
        mixed = [x[1] for x in lv if np.isin(x[4], pile).any() and not np.isin(x[4], pile).all()]
        print(f"f16 + pile, leaf size {leaf}: by count {hist[1:leaf + 1].tolist()}; pile-only leaves {own}, mixed {mixed}")
        assert (hist[1:leaf + 1] > 0).all() and sum(own) + sum(mixed) >= ls.PILE_N
        if leaf >= 5:
            assert max(own) >= 5, own  # a pile leaf of more than one group of four
        if leaf == 16:
            assert sum(1 for c in own if c >= 9) >= 2, own
