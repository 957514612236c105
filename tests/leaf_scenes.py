"""The scene and the export reader of the leaf-size tests (tests/test_oracle_leaf_sizes.py on the CPU,
tests/test_gpu_leaf_sizes.py on the GPU).

The scene is the F-16 (two meshes, 4,056 triangles) and, beside it, the pile: PILE_N congruent triangles
stacked along their normal, PILE_STEP apart. The step is far below the width of a Morton cell of the scene's
box, so the pile's centroids share very few Morton keys, the build cannot tell them apart by position and cuts
them into leaves by count alone: at leaf size 16 the pile fills whole leaves of its own. A ray down the pile's
axis crosses all PILE_N triangles at distinct t, a point on the axis has PILE_N distinct distances, and a box
or a triangle across the pile meets all of them.

leaves() reads the leaf references out of exported node records of any width (BVH2, BVH4, BVH8).
"""
import numpy as np

from raytracercuda_amd import beam, scenes

F = np.float32
EMPTY_REF, LEAF_BIT, FIRST_MASK = 0xFFFFFFFF, 0x80000000, 0x07FFFFFF
LEAF_SIZES = tuple(range(1, 17))
QUERY_LEAF_SIZES = (1, 3, 5, 7, 13, 16)

PILE_N = 40
PILE_STEP = 2.0 ** -12                       # spacing along the normal (+z): exact in float32 at these magnitudes
PILE_AT = (1.25, 0.125, 0.25)                # v0 of the lowest triangle: beside the F-16, inside its y and z range
PILE_TRI = ((0.0, 0.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0))  # the congruent triangle, normal +z
PILE_AXIS = (PILE_AT[0] + 0.0625, PILE_AT[1] + 0.0625)            # x, y of a line through every triangle's interior


def pile_mesh():
    """PILE_N copies of PILE_TRI at PILE_AT + (0, 0, j * PILE_STEP), unindexed, face j the j-th from below."""
    tri = np.asarray(PILE_TRI, np.float64) + np.asarray(PILE_AT, np.float64)
    pos = np.concatenate([tri + [0.0, 0.0, j * PILE_STEP] for j in range(PILE_N)])
    assert np.array_equal(F(pos).astype(np.float64), pos)  # every coordinate exact
    return {"pos": F(pos), "nrm": np.tile(F([0, 0, 1]), (3 * PILE_N, 1)), "idx": np.arange(3 * PILE_N, dtype=np.uint32)}


def f16_meshes():
    return scenes.load_mesh("f16")


def scene_meshes():
    """The F-16's meshes, then the pile: global ids [0, 4056) and [4056, 4096)."""
    return f16_meshes() + [pile_mesh()]


def pile_ids():
    n = sum(np.asarray(m["idx"]).size // 3 for m in f16_meshes())
    return np.arange(n, n + PILE_N, dtype=np.uint32)


def leaves(rec, tris):
    """The leaves a traversal from record 0 reaches in exported node records (16, 32 or 64 words wide):
    (first, count, lo, hi, ids) per leaf — its run in the triangle records, its child box (3,) + (3,) and the
    global ids of its triangles, from word 3 of the triangle records."""
    words = rec.shape[1]
    width = {16: 2, 32: 4, 64: 8}[words]
    box = rec.view(F)
    out = []
    if tris.shape[0] == 0:
        return out
    for node in beam.reachable_records(rec):
        for slot in range(width):
            ref = int(rec[node, 12 + slot] if width == 2 else rec[node, 6 * width + slot])
            if ref == EMPTY_REF or not ref & LEAF_BIT:
                continue
            first, cnt = ref & FIRST_MASK, ((ref >> 27) & 15) + 1
            if width == 2:
                lo, hi = box[node, slot * 6:slot * 6 + 3], box[node, slot * 6 + 3:slot * 6 + 6]
            else:
                lo = box[node, [slot, width + slot, 2 * width + slot]]
                hi = box[node, [3 * width + slot, 4 * width + slot, 5 * width + slot]]
            out.append((first, cnt, lo.copy(), hi.copy(), tris[first:first + cnt, 3].copy()))
    return out


def leaf_histogram(rec, tris):
    """hist[c] = the number of reachable leaves that hold c triangles (index 0 unused), length 17."""
    return np.bincount([lf[1] for lf in leaves(rec, tris)], minlength=17)


def leaf_corners(tris, first, cnt):
    """The 3 * cnt vertices of a leaf's triangle records as the kernels rebuild them: v0, v0 + e1, v0 + e2."""
    t = tris.view(F)[first:first + cnt]
    v0 = t[:, 0:3]
    return np.concatenate([v0, v0 + t[:, 4:7], v0 + t[:, 8:11]])
