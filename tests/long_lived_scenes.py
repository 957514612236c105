"""Walks over objects that live through many calls: one scene rebuilt and refit across the build's size regimes,
one scene whose instances come and go, one render target and camera sent through every trace kernel. Shared by
tests/test_oracle_long_lived.py (what each walk must put in front of the library, asserted from the oracle alone,
without a GPU) and tests/test_gpu_long_lived.py (the walks themselves). Test infrastructure only.

The library keeps state from one call to the next (grow-only buffers, bound replicas that the last reader of a
build zeroes for the next, the per-tile cost table, the ray queue, the shadow plane); a defect there shows only on
the second use of an object, so every step of a walk is made to differ from the one before it in what that state
would carry over: another box, other keys, other pixels.

The regime constants are repeated here as plain numbers with the source line that holds them; neither test reads
the sources.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

F = np.float32

# ---- 1. the build's regimes ------------------------------------------------------------------------------------
CHUNK = 512             # bm_build.hip: constexpr uint32_t REFIT_CHUNK = 1u << REFIT_CHUNK_LOG2 (9)
MSD_MIN_N = 1 << 14     # bm_sort.h: constexpr uint32_t MSD_MIN_N = 1u << 14 (below: the three LSD passes)
PT_MAX_CHUNKS = 256     # bm_build.hip: constexpr uint32_t PT_MAX_CHUNKS = 256 (k_pack4_table up to here)
OSW_SMALL_N = 1 << 17   # bm_sort.h: constexpr uint32_t OSW_SMALL_N = 1u << 17 (the one-sweep tile grows above)
MSD_WIDE_N = 1 << 19    # bm_sort.h: constexpr uint32_t MSD_WIDE_N = 1u << 19 (above: 1,024-lane buckets)
assert PT_MAX_CHUNKS * CHUNK == OSW_SMALL_N  # the table kernel and the sort tile change at the same n

REGIMES = ("empty", "one", "two", "chunk", "lsd", "table", "span", "wide")
# the last reader of the bound replicas, which zeroes them for the next build or refit (BVH4; a BVH2 scene of
# more than one chunk always ends in the chunk-table kernels)
LAST_READER = {"one": "k_pack_small", "two": "k_tree_chunk", "chunk": "k_tree_chunk", "lsd": "k_pack4_table",
               "table": "k_pack4_table", "span": "k_chunk_table_lds", "wide": "k_chunk_table_lds"}


def regime(n):
    """The build's regime for n triangles (host restatement of launch_build / launch_finish)."""
    if n <= 2:
        return REGIMES[n]
    if n <= CHUNK:
        return "chunk"
    if n < MSD_MIN_N:
        return "lsd"
    if n <= PT_MAX_CHUNKS * CHUNK:
        return "table"
    return "span" if n <= MSD_WIDE_N else "wide"


SMALLEST = {"empty": 0, "one": 1, "two": 2, "chunk": 3, "lsd": CHUNK + 1, "table": MSD_MIN_N,
            "span": PT_MAX_CHUNKS * CHUNK + 1, "wide": MSD_WIDE_N + 1}

# n triangles of test_gpu_build_sizes.soup scaled by `scale` and moved by `shift`; kind "skew" is
# test_build_skewed_top_digit's recipe (a dense cluster and one far triangle), "equal" every triangle a copy of
# one (all Morton keys equal). refit: after the build the vertices move out by 4x about the scene centre, are
# refit, move back to a quarter of the original size and are refit again.
Step = namedtuple("Step", "n scale shift kind refit", defaults=((0, 0, 0), "soup", False))
O = (0, 0, 0)
WALK = (
    Step(513, 1.0),
    Step(3, 0.1, O, "soup", True),               # one chunk after several, inside their box
    Step(16384, 1.0, (4, 0, 0), "soup", True),   # top digit first after one chunk
    Step(513, 0.1, (4, 0, 0), "soup", True),     # LSD after top digit first
    Step(131073, 1.0, O, "soup", True),          # table kernel + k_pack4_span after LSD
    Step(524289, 0.1, O, "soup", True),          # the one step above 2^19
    Step(131073, 0.01),
    Step(16384, 0.004),
    Step(2, 0.0015, O, "soup", True),
    Step(513, 1.0, (0, 3, 0)),
    Step(1, 0.1, (0, 3, 0), "soup", True),
    Step(0, 1.0),
    Step(1, 1.0),
    Step(2, 1.0, (0, 0, 3)),
    Step(3, 1.0, (3, 0, 0)),
    Step(16384, 1.0),
    Step(40001, 0.01, O, "skew"),                # after a well-spread scene
    Step(16384, 1.0, (0, -4, 0)),
    Step(20000, 0.1, (0, -4, 0), "equal"),       # after a well-spread scene
)
# the shorter walk (leaf size 1): every small regime and the top-digit-first sort
SHORT_WALK = (
    Step(513, 1.0),
    Step(3, 0.1, O, "soup", True),
    Step(16384, 1.0, (4, 0, 0), "soup", True),
    Step(513, 0.1, (4, 0, 0), "soup", True),
    Step(2, 0.01, (4, 0, 0), "soup", True),
    Step(0, 1.0),
    Step(1, 1.0, O, "soup", True),
    Step(16384, 1.0, (0, 2, 0)),
)
WALKS = {"full": (WALK, 100), "short": (SHORT_WALK, 200)}  # name: (steps, first seed)
FRAME_W, FRAME_H = 64, 48


@lru_cache(maxsize=None)
def step_meshes(walk, i):
    """The meshes of step i of a named walk, built once and shared (never modified). Every step has a seed of its
    own, so consecutive builds share no triangle."""
    from test_gpu_build_sizes import soup

    steps, seed = WALKS[walk]
    s = steps[i]
    if s.n == 0:
        return ()
    n = s.n - 1 if s.kind == "skew" else s.n
    meshes = soup(n, seed=seed + i, dup=n if s.kind == "equal" else 0)
    meshes[0]["pos"] = (meshes[0]["pos"] * F(s.scale) + F(s.shift)).astype(F)
    if s.kind == "skew":
        far = np.array([[100, 100, 100], [101, 100, 100], [100, 101, 100]], F)
        meshes.append({"pos": far, "nrm": np.ones_like(far), "idx": np.arange(3, dtype=np.uint32)})
    for m in meshes:
        for a in m.values():
            a.setflags(write=False)
    return tuple(meshes)


def vertex_box(meshes):
    pos = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3) for m in meshes])
    return pos.min(0), pos.max(0)


def centre_box(meshes):
    """Bounds of the centres of the triangles' boxes: what the Morton keys are quantised over."""
    tri = np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)] for m in meshes])
    cen = (tri.min(1).astype(np.float64) + tri.max(1).astype(np.float64)) / 2
    return cen.min(0), cen.max(0)


def moved(meshes, factor):
    """Every vertex moved to centre + factor * (vertex - centre), centre that of the scene's vertex box."""
    lo, hi = vertex_box(meshes)
    c = ((lo + hi) * F(0.5)).astype(F)
    return tuple(dict(m, pos=(c + (np.asarray(m["pos"], F) - c) * F(factor)).astype(F)) for m in meshes)


def final_meshes(walk, i):
    """What the scene holds when step i is over: the quarter-size vertices after a refit step."""
    m = step_meshes(walk, i)
    return moved(m, 0.25) if WALKS[walk][0][i].refit and m else m


def view(meshes):
    """(eye, window) of the 64 x 48 frame taken of a step: three half-sides in front of the first mesh's box (of
    its first triangle's in a scene of up to three, which would otherwise fall between the pixels)."""
    from raytracercuda_amd import scenes

    if not meshes:
        return (0.1, 0.05, -3.0), scenes.RAYS_SQUARE
    few = sum(np.asarray(m["idx"]).size for m in meshes) <= 9
    lo, hi = vertex_box([dict(meshes[0], pos=np.asarray(meshes[0]["pos"])[:3])] if few else meshes[:1])
    c, r = (lo.astype(np.float64) + hi) / 2, max(float((hi - lo).max()) / 2, 1e-30)
    return tuple(float(v) for v in F([c[0] + 0.1 * r, c[1] + 0.05 * r, c[2] - 3.0 * r])), scenes.RAYS_SQUARE


def own_keys(oracle, meshes, first=0):
    """The oracle's Morton key of every triangle from global id `first` on, in triangle order."""
    rec, tris, keys, perm = oracle.bvh_build(list(meshes), 4, 4).export()
    by_tri = np.empty_like(keys)
    by_tri[perm] = keys
    return by_tri[first:]


def stale_keys(oracle, prev, meshes):
    """The keys of `meshes` over the fold of the previous scene's box with their own: what a build gets whose
    bound replicas still hold the previous build's box (the replicas are folded with max). Where the previous
    box holds this one, that is the previous box itself. By the oracle: it builds both scenes as one."""
    nprev = sum(np.asarray(m["idx"]).size // 3 for m in prev)
    return own_keys(oracle, tuple(prev) + tuple(meshes), nprev)


# ---- 2. instances that come and go ---------------------------------------------------------------------------
def instance_walk():
    """Three lists of (mesh, transform) entries for one scene: instances of two meshes; the first removed and a
    larger mesh's added (the pool offsets move); none (the pools are unused)."""
    from test_gpu_instances import placed, synthetic
    from test_instances_abi import MIRROR, ROTATION, SCALE, rotation

    rng = np.random.default_rng(77)
    a, b, c = synthetic(60, rng), synthetic(257, rng), synthetic(1025, rng)
    x = [placed(ROTATION, (-2.0, 1.0, 0.5)), placed(SCALE, (1.5, -1.2, 0.5)), placed(MIRROR, (2.0, 1.5, 1.0)),
         placed(rotation((3, -1, 2), 1.9), (-1.5, -1.5, 0.25))]
    first = [(a, x[0]), (b, x[1]), (a, x[2])]
    second = first[1:] + [(c, x[3])]
    return first, second, []


INSTANCE_EYE = (0.0, 0.0, -4.5)
QUERY_N = 257


def query_batch(meshes, seed):
    """257 rays from one origin outside the box, 257 segments and 257 points in and around it."""
    rng = np.random.default_rng(seed)
    if meshes:
        lo, hi = (v.astype(np.float64) for v in vertex_box(meshes))
    else:
        lo, hi = -np.ones(3), np.ones(3)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    u = rng.normal(size=3)
    eye = F(c + 0.9 * ext * u / np.linalg.norm(u))
    o = np.tile(eye, (QUERY_N, 1))
    d = F(c + rng.uniform(-0.6, 0.6, (QUERY_N, 3)) * (hi - lo)) - eye + F(0.0)
    a = F(c + rng.uniform(-0.75, 0.75, (QUERY_N, 3)) * (hi - lo))
    b = F(c + rng.uniform(-0.75, 0.75, (QUERY_N, 3)) * (hi - lo))
    pts = F(c + rng.uniform(-0.9, 0.9, (QUERY_N, 3)) * (hi - lo))
    return o, d, a, b, pts


# ---- 3. one render target through every kernel kind --------------------------------------------------------------
W, H = 136, 72          # 17 x 9 cull tiles: 39 regions of 4, 5 of 36 (the last one partial); 4.5 bands of 16 rows
QUAD_TILES = ((W + 3) // 4) * ((H + 3) // 4)
SENTINEL = 0xFFABCDEF   # packed colours are 0x00RRGGBB: no shading produces it
LANES, QUAD, COMPACT, PACKET = 6, 10, 12, 14  # bm_internal.h TraceVariant
LIGHT_A, LIGHT_B = (0.0, 10.0, -10.0), (-6.0, -2.0, -8.0)
WINDOWS = {"square": (-1.0, 1.0, -1.0, 1.0, 1.0), "other": (-0.6, 1.1, -0.9, 0.8, 1.3)}
D0, D1, D2, D3 = (0.1, 0.05, -1.25), (-0.3, 0.2, -1.15), (0.3, -0.2, -1.4), (-0.15, -0.3, -1.2)
W0, W1, W2 = (2.885, 0.5, -0.3), (2.86, -1.0, -0.25), (2.9, 1.7, -0.4)
BANDS = (16, 3, 1)      # band height, ranks, this rank: bands 1 and 4 of 5, 32 local rows of the 72

# mode: "trace", "count" (a counting trace), "bands"; cost: the table written before the step; w, h, target: the
# camera's frame and the target traced into ("big": 136 x 72, "small": 64 x 64); kind: what traceKind() must say
Frame = namedtuple("Frame", "scene eye variant sched tiles light mode cost kind window w h target",
                   defaults=(None, "trace", None, "quads", "square", W, H, "big"))
SEQUENCE = (
    Frame("dense", D0, QUAD, 1, 4),
    Frame("wire", W0, COMPACT, 1, 4, kind="cull+quads"),
    Frame("dense", D1, PACKET, 1, 4, kind="packets"),
    Frame("wire", W1, LANES, 1, 4, kind="lanes"),
    Frame("dense", D2, QUAD, 2, 4, LIGHT_A, cost="descending"),
    Frame("wire", W2, COMPACT, 1, 36, LIGHT_A, kind="cull+quads"),
    Frame("dense", D3, PACKET, 1, 36, mode="count"),                     # counting: the quad kernel
    Frame("wire", W0, PACKET, 1, 36, kind="packets"),
    Frame("dense", D0, COMPACT, 1, 4, cost="constant", kind="cull+quads"),
    Frame("wire", W1, QUAD, 2, 4),                                      # the table as the last kernels left it
    Frame("dense", D1, LANES, 1, 4, LIGHT_B, kind="lanes"),
    Frame("wire", W2, QUAD, 1, 4, mode="bands"),
    Frame("dense", D2, QUAD, 1, 4),
    Frame("wire", W0, COMPACT, 1, 4, kind="cull+quads", window="other"),
    Frame("dense", D3, PACKET, 1, 4, kind="packets", window="other"),
    Frame("wire", W1, QUAD, 2, 4, w=64, h=64, target="small"),
    Frame("dense", D0, QUAD, 2, 4, LIGHT_A, cost="descending"),
    Frame("wire", W2, COMPACT, 1, 36, mode="bands", kind="cull+quads"),
    Frame("dense", D1, QUAD, 2, 4, mode="count"),
    Frame("wire", W0, LANES, 1, 4, LIGHT_B, kind="lanes"),
)
# the context with queued shadow rays (BM_OPT_SHADOW_QUEUE): its shadow trace is the single-lane kernels'
QUEUE_SEQUENCE = (
    Frame("dense", D0, QUAD, 1, 4, LIGHT_A, kind="lanes"),
    Frame("wire", W0, QUAD, 1, 4),
    Frame("dense", D2, QUAD, 1, 4, LIGHT_B, kind="lanes"),
)


def cost_table(name):
    if name == "descending":
        return np.arange(QUAD_TILES, 0, -1, dtype=np.uint32) * np.uint32(1000)
    return np.full(QUAD_TILES, 77777, np.uint32)


def frame_planes(oracle, fr):
    """The oracle's planes and counters of a frame of a sequence (test_gpu_ray_queue.expected: shared)."""
    from test_gpu_ray_queue import expected

    return expected(oracle, fr.scene, fr.w, fr.h, eye=fr.eye, light=fr.light, cam=WINDOWS[fr.window])


def band_rows(h, band_h, step, first):
    """[(local row, global rows)] of a rank's bands."""
    mine = [b for b in range((h + band_h - 1) // band_h) if b % step == first]
    return [(i * band_h, slice(b * band_h, min((b + 1) * band_h, h))) for i, b in enumerate(mine)]


# three targets in flight: 12 frames, odd ones (counted from 1) of the wire, even ones of the dense scene,
# which is refit between frames 6 and 7
FLIGHT_EYES = {"dense": (D0, D1, D2), "wire": (W0, W1, W2)}
FLIGHT_FRAMES = 12


def flight_scene(k):
    """Scene of frame k (counted from 1)."""
    return "wire" if k % 2 else "dense"


def dense_moved():
    from test_gpu_ray_queue import SCENES
    from test_gpu_refit import wobble

    return wobble(SCENES["dense"], 0.3, 1.0)
