"""orc_kd_leaves (CPU): the kd oracle's leaves as (path key, count, stored faces), the list the GPU's
reference-mode tree is compared with leaf by leaf (tests/test_gpu_kd_export.py)."""
import numpy as np
import pytest

from raytracercuda_amd import scenes

ONE_LEAF = np.array([[.101, .101, .101], [.102, .101, .101], [.101, .102, .101]], np.float32)
BIG = np.array([[-5, -5, .3], [5, -5, .3], [0, 5, .9]], np.float32)


def soup(*tris):
    pos = np.concatenate([np.asarray(t, np.float32).reshape(-1, 3) for t in tris])
    nrm = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (pos.shape[0], 1))
    return [{"pos": pos, "nrm": nrm, "idx": np.arange(pos.shape[0], dtype=np.uint32)}]


def path_key(p, depth):
    """The path of the depth-`depth` cell holding point p: the world box ±30 halved in float32 along
    axis d % 3, right = 1, depth 0 in the highest bit (p on no split plane)."""
    mn, mx = np.full(3, -30.0, np.float32), np.full(3, 30.0, np.float32)
    key = 0
    for d in range(depth):
        a = d % 3
        s = np.float32(0.5) * (mn[a] + mx[a])
        right = p[a] > s
        assert p[a] != s
        key = (key << 1) | int(right)
        if right:
            mn[a] = s
        else:
            mx[a] = s
    return key


def check_sums(kd):
    keys, counts, faces, depth = kd.leaves()
    st = kd.stats()
    assert keys.dtype == counts.dtype == faces.dtype == np.uint32
    assert (np.diff(keys.astype(np.int64)) > 0).all()  # strictly ascending
    assert (counts > 0).all()
    c = counts.astype(np.int64)
    assert int(np.minimum(c, 256).sum()) == int(st[2]) == faces.size
    assert int(np.maximum(c - 256, 0).sum()) == int(st[3])
    assert int(c.max(initial=0)) == int(st[4])
    return keys, counts, faces, depth, st


@pytest.mark.parametrize("name", ["suzanne", "f16"])
def test_leaves_of_a_mesh(oracle, name):
    meshes = scenes.load_mesh(name)
    keys, counts, faces, depth, st = check_sums(oracle.kd_build(meshes))
    assert depth == 31 and keys.size > 100 and int(keys.max()) < 2 ** 31
    n = sum(m["idx"].size // 3 for m in meshes)
    assert int(faces.max()) < n
    # insertion order is ascending triangle id: every leaf's stored list ascends
    start = np.concatenate([[0], np.cumsum(np.minimum(counts, 256))[:-1]]).astype(np.int64)
    inner = np.ones(faces.size, bool)
    inner[start] = False
    assert (np.diff(faces.astype(np.int64))[inner[1:]] > 0).all()
    # every triangle's centroid cell is one of its leaves, unless the cap dropped the triangle there
    tri = np.concatenate([m["pos"][m["idx"].reshape(-1, 3)] for m in meshes])
    leaf_of = np.repeat(np.arange(keys.size), np.minimum(counts, 256))
    for g in range(0, n, max(1, n // 64)):
        ctr = (tri[g].astype(np.float64).sum(0) / 3).astype(np.float32)
        k = path_key(ctr, depth)
        i = int(np.searchsorted(keys, k))
        assert i < keys.size and keys[i] == k, (g, k)
        assert g in faces[leaf_of == i] or counts[i] > 256


def test_one_leaf_has_the_key_of_its_cell(oracle):
    keys, counts, faces, depth, st = check_sums(oracle.kd_build(soup(ONE_LEAF)))
    assert depth == 31
    assert keys.tolist() == [path_key(ONE_LEAF[0], 31)] and counts.tolist() == [1] and faces.tolist() == [0]


def test_leaf_cap_keeps_counting(oracle):
    keys, counts, faces, depth, st = check_sums(oracle.kd_build(soup(*[ONE_LEAF] * 300)))
    assert keys.tolist() == [path_key(ONE_LEAF[0], 31)] and counts.tolist() == [300]
    assert faces.tolist() == list(range(256)) and int(st[3]) == 44


def test_childless_nodes_are_not_leaves(oracle):
    """One large triangle passes box tests of nodes whose children it both misses: orc_kd_stats[1] counts
    those childless nodes, orc_kd_leaves only the leaves that hold the face."""
    keys, counts, faces, depth, st = check_sums(oracle.kd_build(soup(BIG)))
    assert (counts == 1).all() and (faces == 0).all()
    assert keys.size == int(st[2]) == 31663 and int(st[1]) == 31664


def test_no_leaves(oracle):
    out = soup(ONE_LEAF + np.float32(100.0))
    keys, counts, faces, depth, st = check_sums(oracle.kd_build(out))
    assert keys.size == counts.size == faces.size == 0 and depth == 0
