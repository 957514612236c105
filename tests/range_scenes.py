"""Scenes and views that stretch the range of the coordinates: far eyes, large world offsets, very small and
very large scales. Shared by tests/test_oracle_range.py (the oracle's BVH against its brute force, without
a GPU) and tests/test_gpu_range.py (every trace path against the oracle's BVH). Test infrastructure only.

Every other GPU test compares a kernel with the oracle's BVH trace, which shares the kernels' slab test, box
padding and tie rule; a loss of conservativeness common to both would pass. Here the oracle's BVH is itself
compared with the exhaustive trace over a grid of views, and the GPU with both.

A scene is centred on the origin with extent 1 (the side of its box; see suzanne()). A view (D, direction, T,
S) places it at pos*S + T*OFFSET (computed in double, rounded to float32), the eye at the same transform of
D*dir, looks at the scene's centre and opens the camera window to +-0.9/D, so the scene fills the same share
of the frame at every D. The light is the same transform of 1.5*D*LIGHT_DIR.

D_OK is the largest eye distance (in scene extents, a power of two of the grid) at which the oracle's BVH
equals brute force on every scene, direction and BVH width: measured by tests/test_oracle_range.py on the
oracle alone, never with a GPU.
"""
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from deep_scenes import look
from raytracercuda_amd import scenes

MISS = np.uint32(0xFFFFFFFF)
W = H = 192
OFFSET = np.array([1.0, 0.7, -0.4])
LIGHT_DIR = np.array([-0.5, 0.6, -0.62]) / np.linalg.norm([-0.5, 0.6, -0.62])
SCENES = ("cube", "soup", "suzanne")
# eye directions (unit vectors from the scene's centre to the eye): exactly axial (identity orientation,
# two zero direction components in the central column and row of rays), one zero component, two general
DIRS = {"axial": (0.0, 0.0, -1.0), "zero-y": (0.6, 0.0, -0.8), "diag": (1.0, 1.0, 1.0),
        "oblique": (-0.3, 0.8, 0.52)}
D_GRID = (3, 8, 16, 32, 64, 128, 256, 1024, 4096, 32768)
T_GRID = (1e3, 1e5, 1e6)
S_EXP = (-60, -30, -10, 10, 30, 40, 42, 44, 50, 60)   # S = 2^k
D_OK = 32
S_OK = (-30, 30)   # the scales of the envelope, as exponents


def view_id(v):
    return f"D{v.D}-{v.dir}-T{v.T:g}-S2^{v.s_exp}"


def _views():
    out = []
    for d in DIRS:
        out += [SimpleNamespace(D=D, dir=d, T=0.0, s_exp=0) for D in D_GRID]
        out += [SimpleNamespace(D=3, dir=d, T=T, s_exp=0) for T in T_GRID]
        out += [SimpleNamespace(D=3, dir=d, T=0.0, s_exp=k) for k in S_EXP]
    for v in out:
        v.id = view_id(v)
    return out


VIEWS = _views()
BY_ID = {v.id: v for v in VIEWS}
def views_of(scene):
    """The views a scene is traced from: the whole grid, for every scene."""
    return VIEWS


def inside(v):
    """The envelope: any offset, scales 2^-30 .. 2^30, the eye within D_OK extents."""
    return v.D <= D_OK and S_OK[0] <= v.s_exp <= S_OK[1]


# ---- scenes at extent 1 around the origin -------------------------------------------------------------
def _unshared(tris, seed):
    """One mesh of unshared vertices; random vertex normals, so packed colours differ between triangles."""
    p = np.asarray(tris, np.float64).reshape(-1, 3)
    nrm = np.random.default_rng(seed).normal(size=p.shape).astype(np.float32)
    return [{"pos": p, "nrm": nrm, "idx": np.arange(p.shape[0], dtype=np.uint32)}]


def cube(k=16):
    """The axis-aligned cube [-0.5, 0.5]^3 with k x k quads (2 triangles each) per face: 12 k^2 triangles."""
    g = np.arange(k + 1) / k - 0.5
    tris = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (-0.5, 0.5):
            for i in range(k):
                for j in range(k):
                    q = np.zeros((4, 3))
                    q[:, axis] = side
                    q[:, a] = (g[i], g[i + 1], g[i + 1], g[i])
                    q[:, b] = (g[j], g[j], g[j + 1], g[j + 1])
                    tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
    return _unshared(tris, 11)


def soup(n=3000, sigma=0.05, seed=2024):
    """n triangles: centres uniform in [-0.5, 0.5]^3, vertices the centre plus normal jitter of sigma."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 0.5, (n, 1, 3))
    return _unshared(c + rng.normal(0.0, sigma, (n, 3, 3)), 12)


def suzanne():
    """The committed suzanne mesh, centred and scaled so that the smallest side of its box is 1 (the largest
    is 1.59): with the largest at 1 it covers an eighth of the frame, half of the quarter that the frame
    sanity checks ask of every view. Its D therefore counts in units of 0.63 of its largest side (D = 32 is
    20 of those); the cube and the soup are the scenes of extent exactly 1 that D_OK rests on."""
    meshes = scenes.load_mesh("suzanne")
    pos = np.concatenate([np.asarray(m["pos"], np.float64) for m in meshes])
    lo, hi = pos.min(0), pos.max(0)
    c, ext = (lo + hi) / 2, float((hi - lo).min())
    return [{"pos": (np.asarray(m["pos"], np.float64) - c) / ext, "nrm": m["nrm"], "idx": m["idx"]} for m in meshes]


_UNIT, _MESHES, _BVH, _RAYS, _BVH_FRAMES, _BRUTE = {}, {}, {}, {}, {}, {}
_MAKE = {"cube": cube, "soup": soup, "suzanne": suzanne}


def place(p, T, s_exp):
    """pos*S + T*OFFSET in double, rounded to float32 (S = 2^s_exp: the product is exact)."""
    return np.float32(np.asarray(p, np.float64) * 2.0 ** s_exp + T * OFFSET)


def meshes_of(scene, T=0.0, s_exp=0):
    """The scene placed at (T, S): float32 positions, the unit scene's normals and indices."""
    if scene not in _UNIT:
        _UNIT[scene] = _MAKE[scene]()
    key = (scene, T, s_exp)
    if key not in _MESHES:
        _MESHES[key] = [{"pos": place(m["pos"], T, s_exp), "nrm": m["nrm"], "idx": m["idx"]} for m in _UNIT[scene]]
    return _MESHES[key]


def camera(v):
    """(left, right, top, bottom, zoom) of the view's camera window."""
    r = 0.9 / v.D
    return (-r, r, r, -r, 1.0)


def eye_of(v):
    d = np.asarray(DIRS[v.dir], np.float64)
    return place(v.D * d / np.linalg.norm(d), v.T, v.s_exp)


def orient_of(v):
    return look(-np.asarray(DIRS[v.dir], np.float64))


def light_of(v):
    return place(1.5 * v.D * LIGHT_DIR, v.T, v.s_exp)


def rays_of(oracle, v):
    if v.D not in _RAYS:
        err, rays = oracle.camera_rays(W, H, *camera(v))
        assert err == 0
        rays.setflags(write=False)
        _RAYS[v.D] = rays
    return _RAYS[v.D]


def _frozen(a):
    a.setflags(write=False)
    return a


def oracle_bvh(oracle, scene, T, s_exp, width):
    key = (scene, T, s_exp, width)
    if key not in _BVH:
        _BVH[key] = oracle.bvh_build(meshes_of(scene, T, s_exp), 4, width)
    return _BVH[key]


# ---- the oracle's answers, computed once per process and left unchanged (arrays are read-only) ----------
def bvh_expected(oracle, scene, v, width=4):
    """The oracle's BVH answers of a view at leaf size 4: .frame {"packed", "tri_id", "t", "shadow"}, .cnt
    (the three trace counters, then the three shadow counters), .eye, .orient, .light, .rays."""
    key = (scene, v.id, width)
    if key not in _BVH_FRAMES:
        obvh = oracle_bvh(oracle, scene, v.T, v.s_exp, width)
        rays, eye, orient, light = rays_of(oracle, v), eye_of(v), orient_of(v), light_of(v)
        packed, tri, t, cnt = obvh.render(rays, eye, orient, counters=True)
        sh, scnt = obvh.shadow(rays, eye, orient, light, tri, t, counters=True)
        frame = {"packed": _frozen(packed), "tri_id": _frozen(tri), "t": _frozen(t), "shadow": _frozen(sh)}
        _BVH_FRAMES[key] = SimpleNamespace(frame=frame, cnt=_frozen(np.concatenate([cnt, scnt])), eye=eye,
                                           orient=orient, light=light, rays=rays)
    return _BVH_FRAMES[key]


def brute_expected(oracle, scene, v):
    """The exhaustive answers of a view: {"packed", "tri_id", "t", "shadow"} (the shadow rays start from the
    exhaustive frame's own hits)."""
    key = (scene, v.id)
    if key not in _BRUTE:
        m = meshes_of(scene, v.T, v.s_exp)
        rays, eye, orient = rays_of(oracle, v), eye_of(v), orient_of(v)
        packed, tri, t = oracle.brute_render(m, rays, eye, orient)
        sh = oracle.brute_shadow(m, rays, eye, orient, light_of(v), tri, t)
        _BRUTE[key] = {"packed": _frozen(packed), "tri_id": _frozen(tri), "t": _frozen(t), "shadow": _frozen(sh)}
    return _BRUTE[key]


def warm(oracle, pairs, widths=(), brute=True):
    """Compute the exhaustive answers (and the BVH answers at `widths`) of (scene, view) pairs on several
    threads: the oracle's calls release the interpreter lock and share no state."""
    for s, v in pairs:  # the shared inputs first, on this thread
        rays_of(oracle, v)
        for w in widths:
            oracle_bvh(oracle, s, v.T, v.s_exp, w)
    jobs = [lambda s=s, v=v: brute_expected(oracle, s, v) for s, v in pairs if brute]
    jobs += [lambda s=s, v=v, w=w: bvh_expected(oracle, s, v, w) for s, v in pairs for w in widths]
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        list(pool.map(lambda job: job(), jobs))


def clear():
    """Drop every cached answer (a test module calls this when it is done: the frames of the whole grid
    are a few hundred MB)."""
    for cache in (_MESHES, _BVH, _RAYS, _BVH_FRAMES, _BRUTE):
        cache.clear()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(a, b):
    """Pixels of frame a (the BVH's) that differ from frame b (the exhaustive one): ids, lost hits (a misses
    where b hits), t bits, packed colours, shadow bytes."""
    return {"ids": int((a["tri_id"] != b["tri_id"]).sum()),
            "lost": int(((a["tri_id"] == MISS) & (b["tri_id"] != MISS)).sum()),
            "t": int((bits(a["t"]) != bits(b["t"])).sum()),
            "packed": int((a["packed"] != b["packed"]).sum()),
            "shadow": int((a["shadow"] != b["shadow"]).sum())}


def hit_is_finite_t(f):
    """A frame's hits are exactly its pixels with a finite t > 0 (a miss carries +inf)."""
    t, hit = f["t"], f["tri_id"] != MISS
    return bool(np.array_equal(hit, np.isfinite(t) & (t > 0)) and np.all(np.isposinf(t[~hit])))


def overflowing(oracle, scene, v):
    """Pixels of an S > 1 view whose S = 1 hit overflows at S: the same ray against the same triangle, scaled
    (an exact operation, so without overflow every intermediate is the S = 1 one times a power of two),
    returns a non-finite t from the oracle's own triangle test (orc_pin_ops)."""
    from test_gpu_rays import pin_uv, tri_vertices
    base = SimpleNamespace(D=v.D, dir=v.dir, T=v.T, s_exp=0)
    base.id = view_id(base)
    tri = brute_expected(oracle, scene, base)["tri_id"]
    hit = np.flatnonzero(tri != MISS)
    rays, orient = rays_of(oracle, v), orient_of(v).reshape(3, 3)  # column-major: dir = orient^T-of-rows
    d = np.float32((rays[hit, 0:1] * orient[0] + rays[hit, 1:2] * orient[1]) + rays[hit, 2:3] * orient[2])
    o = np.broadcast_to(eye_of(v), d.shape)
    t, _, _ = pin_uv(oracle, np.ascontiguousarray(o), d, tri_vertices(meshes_of(scene, v.T, v.s_exp)), tri[hit])
    return int((~np.isfinite(t)).sum()), hit.size
