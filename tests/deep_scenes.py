"""Scenes whose rays need a deep traversal stack, shared by tests/test_oracle_deep_stack.py (which checks
the fixture and the oracle on it, without a GPU) and tests/test_gpu_stack_overflow.py (which traces it
with every ray kernel). Test infrastructure only.

"deep" is the chain of tests/test_gpu_points.py's deep_scene with large triangles: centres whose 30-bit
Morton keys are 0, every single bit 2^k (five triangles each) and the all-ones key, so the Karras tree
is a chain towards key 0; the triangles span +-2048 around their centres, so a ray through the scene
hits the box of every sibling on the chain and has to keep all of them on its stack. "deep+dup" adds
copies of the triangle at the origin: equal keys and the highest ids, a balanced subtree below the
chain's end. Every ray kernel keeps at most 24 stack entries per ray in LDS (QUAD_LDS; 8, 12 or 16 in
the single-lane kernels); these scenes need 30 to 63, so the rest live in the global overflow area.
"""
from types import SimpleNamespace

import numpy as np

H = 2048.0
QUAD_LDS = 24           # LDS stack entries per ray of the quad and ray-query kernels
LANE_LDS = (12, 16)     # ... of the single-lane kernels (trace_variant_lds), reported only
MAX_STACK = 96          # rows of the overflow area (bm_api.cpp reserve_overflow), LDS entries included
MISS = np.uint32(0xFFFFFFFF)
CAM = (-1.0, 1.0, 1.0, -1.0, 1.0)   # Oracle.camera_rays' default frustum
LIGHT = (900.0, -2500.0, 300.0)
IDENTITY = np.eye(3, dtype=np.float32).reshape(9)
ONE_RAY = np.float32([[0.0, 0.0, 1.0]])


def deep_vertices(dup=0):
    """(ntri, 3, 3) float32 vertices: 152 chain triangles, then `dup` copies of the one at the origin."""
    shape = np.array([[-H, -H, -H], [H, H, H], [H, -H, 0.0]])
    centres = [np.zeros(3), np.full(3, 1024.0)]
    for axis in range(3):
        for j in range(10):
            c = np.full(3, 0.25)
            c[axis] = 2.0 ** j + 0.5
            centres += [c] * 5
    centres += [np.zeros(3)] * dup
    return np.float32(np.asarray(centres)[:, None, :] + shape[None, :, :])


def deep_meshes(dup=0):
    """The scene as one unshared mesh; random vertex normals, so packed colours differ between triangles."""
    v = deep_vertices(dup).reshape(-1, 3)
    nrm = np.random.default_rng(1000 + dup).normal(size=v.shape).astype(np.float32)
    return [{"pos": v, "nrm": nrm, "idx": np.arange(v.shape[0], dtype=np.uint32)}]


def look(fwd, up=(0.0, 1.0, 0.0)):
    """Column-major mat3 (right, up, forward) of a camera looking along fwd."""
    f = np.asarray(fwd, np.float64)
    f = f / np.linalg.norm(f)
    right = np.cross(np.asarray(up, np.float64), f)
    right /= np.linalg.norm(right)
    up = np.cross(f, right)
    return np.stack([right, up, f], 1).astype(np.float32).T.reshape(-1)


# (eye, orient): along +x every ray is deep. Along the diagonal about a quarter are and the rest are
# shallow, so deep and shallow rays share a wave, but only 2 to 3 % of its rays hit anything. "mixed"
# is deep for about half of its rays and hits with a fifth of them.
VIEWS = {"axis": ((-3000.0, 500.0, 500.0), look((1, 0, 0))),
         "diag": ((-3000.0, -3100.0, -3200.0), look((1, 1, 1))),
         "mixed": ((-4000.0, -1000.0, 500.0), look((1, -0.5, 0)))}
# Frames in flight on several streams look along three different axes: their rays order the chain's
# siblings differently, so at the same depth their stacks hold different entries, and an entry that
# strayed into another stream's area would not go unnoticed.
FLIGHT_VIEWS = {"axis": VIEWS["axis"],
                "along_y": ((500.0, -3000.0, 500.0), look((0, 1, 0), up=(0, 0, 1))),
                "along_z": ((-1500.0, -1500.0, -3000.0), look((0.3, 0, 1)))}
ALL_VIEWS = {**VIEWS, **FLIGHT_VIEWS}
# Origins of the query rays, dealt round-robin, for the same reason: the 16 rays of a wave then carry
# four different stacks.
QUERY_ORIGINS = np.float32([FLIGHT_VIEWS["axis"][0], FLIGHT_VIEWS["along_y"][0], FLIGHT_VIEWS["along_z"][0],
                            (-2500.0, -2600.0, -2700.0)])

# (name, copies of the origin triangle, leaf size) of the scenes the GPU tests trace
SCENES = [("deep", 0, 4), ("deep+dup-leaf1", 1024, 1), ("deep+dup-leaf4", 4096, 4)]
SIZES = [(64, 48), (37, 23)]


def ray_batch(n=1999, seed=5):
    """Closest-hit query rays (origins, dirs) from QUERY_ORIGINS in turn into the box [-200, 1200]^3.
    n is odd on purpose: no multiple of 16."""
    rng = np.random.default_rng(seed)
    targets = np.float32(rng.uniform(-200.0, 1200.0, (n, 3)))
    o = QUERY_ORIGINS[np.arange(n) % QUERY_ORIGINS.shape[0]].copy()
    return o, (targets - o) + np.float32(0.0)


def shallow_rays(n, seed=6):
    """Rays that miss the scene's box (they start beyond it and point away): their stacks stay empty."""
    rng = np.random.default_rng(seed)
    o = np.float32(rng.uniform(5000.0, 6000.0, (n, 3)))
    d = np.float32(rng.uniform(0.1, 1.0, (n, 3)))
    return o, d


def segments(n=1200, seed=8):
    """Any-hit segments (a, b, d = b - a) with both ends in the box [-2500, 3500]^3, kept where a + d
    gives b back exactly (the oracle takes the end point, the GPU the direction)."""
    rng = np.random.default_rng(seed)
    a = np.float32(rng.uniform(-2500.0, 3500.0, (2 * n, 3)))
    b = np.float32(rng.uniform(-2500.0, 3500.0, (2 * n, 3)))
    d = b - a
    exact = np.all(a + d == b, axis=1)
    return a[exact][:n], b[exact][:n], d[exact][:n]


def frame_stats(tri, depth, shadow=None, sdepth=None):
    """The figures both test files report: deepest stack, share of rays beyond 12/16/24 entries, hit
    fraction, distinct triangles hit and, with a light, the shadowed share of hit pixels and the share
    of cast shadow rays beyond 24."""
    hit = tri != MISS
    s = {"deepest": int(depth.max()), "hit": float(hit.mean()), "distinct": int(np.unique(tri[hit]).size)}
    for k in LANE_LDS + (QUAD_LDS,):
        s[f">{k}"] = float((depth > k).mean())
    if shadow is not None:
        s["shadowed"] = float(shadow[hit].mean()) if hit.any() else 0.0
        s["shadow_deepest"] = int(sdepth.max())
        s["shadow>24"] = float((sdepth[hit] > QUAD_LDS).mean()) if hit.any() else 0.0
    return s


def fmt(s):
    return ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in s.items())


# ---- the oracle's answers, computed once per process and left unchanged (arrays are read-only) ----------
_BVH, _FRAMES = {}, {}


def scene_of(name):
    return next(s for s in SCENES if s[0] == name)


def oracle_bvh(oracle, name, width=4):
    """(meshes, OrcBVH) of a scene of SCENES at its leaf size."""
    if (name, width) not in _BVH:
        _, dup, leaf = scene_of(name)
        meshes = deep_meshes(dup)
        _BVH[name, width] = (meshes, oracle.bvh_build(meshes, leaf, width))
    return _BVH[name, width]


def _frozen(a):
    a.setflags(write=False)
    return a


def expected(oracle, name, width, view, size, light=None):
    """The oracle's frame of a scene from a view of ALL_VIEWS at size = (w, h): .frame {"packed", "tri_id",
    "t"[, "shadow"]}, .cnt (3 counters, 6 with a light), .eye, .orient,
    .depth / .sdepth (deepest stack per primary / shadow ray), .stats (frame_stats), .rays."""
    key = (name, width, view, size, light)
    if key not in _FRAMES:
        _, obvh = oracle_bvh(oracle, name, width)
        eye_, orient = ALL_VIEWS[view]
        err, rays = oracle.camera_rays(*size, *CAM)
        assert err == 0
        n = rays.shape[0]
        depth = np.zeros(n, np.uint32)
        packed, tri, t, cnt = obvh.render(rays, eye_, orient, counters=True, depth=depth)
        frame = {"packed": _frozen(packed), "tri_id": _frozen(tri), "t": _frozen(t)}
        sh = sdepth = None
        if light is not None:
            sdepth = np.zeros(n, np.uint32)
            sh, scnt = obvh.shadow(rays, eye_, orient, light, tri, t, counters=True, depth=sdepth)
            frame["shadow"] = _frozen(sh)
            cnt = np.concatenate([cnt, scnt])
            _frozen(sdepth)
        _FRAMES[key] = SimpleNamespace(frame=frame, cnt=_frozen(cnt), depth=_frozen(depth), sdepth=sdepth,
                                       stats=frame_stats(tri, depth, sh, sdepth), rays=rays, eye=eye_,
                                       orient=orient)
    return _FRAMES[key]


def closest_expected(oracle, obvh, meshes, o, d):
    """Closest-hit answers {"t", "u", "v", "tri_id"}, summed counters and per-ray deepest stack of query
    rays (o, d): one oracle trace per distinct origin; u and v from orc_pin_ops on the winning triangle,
    as in tests/test_gpu_rays.py."""
    from test_gpu_rays import pin_uv, tri_vertices
    n = o.shape[0]
    tri, t = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    depth = np.zeros(n, np.uint32)
    cnt = np.zeros(3, np.uint64)
    origins, inverse = np.unique(o, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for g in range(origins.shape[0]):
        sel = np.flatnonzero(inverse == g)
        dep = np.zeros(sel.size, np.uint32)
        _, tri[sel], t[sel], c = obvh.render(d[sel], origins[g], IDENTITY, counters=True, depth=dep)
        depth[sel] = dep
        cnt += c
    hit = tri != MISS
    u, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if hit.any():
        pt, u[hit], v[hit] = pin_uv(oracle, o[hit], d[hit], tri_vertices(meshes), tri[hit])
        assert np.array_equal(pt.view(np.uint32), t[hit].view(np.uint32))
    return {"t": t, "u": u, "v": v, "tri_id": tri}, cnt, depth


def anyhit_expected(obvh, a, b):
    """Occlusion bytes, summed counters and per-segment deepest stack of the segments a[i] -> b[i] (one
    oracle call each: a primary t of 0 makes the shadow origin the eye and light - eye the segment)."""
    n = a.shape[0]
    occ, depth = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    cnt = np.zeros(3, np.uint64)
    zero_tri, zero_t, dep = np.zeros(1, np.uint32), np.zeros(1, np.float32), np.zeros(1, np.uint32)
    for i in range(n):
        s, c = obvh.shadow(ONE_RAY, a[i], IDENTITY, b[i], zero_tri, zero_t, counters=True, depth=dep)
        occ[i], depth[i] = s[0], dep[0]
        cnt += c
    return occ, cnt, depth


QUERY_SCENES = ["deep", "deep+dup-leaf1"]  # ray queries need BVH4
MIXED_PAIRS = 500
_QUERIES = {}


def query_expected(oracle, name):
    """The query batches of a scene and the oracle's answers: the closest-hit batch (.o, .d, .exp, .cnt,
    .depth), its first MIXED_PAIRS rays interleaved one by one with shallow rays (.mix_*), and the any-hit
    segments (.a, .b, .seg_d, .occ, .seg_cnt, .seg_depth)."""
    if name not in _QUERIES:
        meshes, obvh = oracle_bvh(oracle, name, 4)
        o, d = ray_batch()
        exp, cnt, depth = closest_expected(oracle, obvh, meshes, o, d)
        so, sd = shallow_rays(MIXED_PAIRS)
        mo, md = np.empty((2 * MIXED_PAIRS, 3), np.float32), np.empty((2 * MIXED_PAIRS, 3), np.float32)
        mo[0::2], mo[1::2], md[0::2], md[1::2] = o[:MIXED_PAIRS], so, d[:MIXED_PAIRS], sd
        mexp, mcnt, mdepth = closest_expected(oracle, obvh, meshes, mo, md)
        a, b, seg_d = segments()
        occ, scnt, sdepth = anyhit_expected(obvh, a, b)
        _QUERIES[name] = SimpleNamespace(o=o, d=d, exp=exp, cnt=cnt, depth=depth, mix_o=mo, mix_d=md, mix_exp=mexp,
                                         mix_cnt=mcnt, mix_depth=mdepth, a=a, b=b, seg_d=seg_d, occ=occ,
                                         seg_cnt=scnt, seg_depth=sdepth)
    return _QUERIES[name]


def query_stats(depth, hit):
    """deepest stack, share of rays beyond 12/16/24 entries and hit (or occluded) fraction of a batch."""
    s = {"deepest": int(depth.max()), "hit": float(np.mean(hit))}
    for k in LANE_LDS + (QUAD_LDS,):
        s[f">{k}"] = float((depth > k).mean())
    return s
