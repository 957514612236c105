"""Sphere-cast queries (bm_scene_sweep_spheres): the swept-sphere function restated, the brute force, which
candidate wins where, the function's quality against float64 geometry, the conservativeness of the traversal's
node test walked over the oracle's BVH4 without a GPU, the ABI's layout and null handling, the C++ layer (CPU).

The yardstick is brute_force_sweep: tri_sweep below (the header's function in numpy float32, one rounding per
operation, in the order written; its start is test_points_abi.tri_nearest) evaluated for every triangle and
every valid sweep, the lexicographic minimum of (t, id). No value in it comes from the library.
"""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from raytracercuda_amd import _lib, scenes
from test_points_abi import tri_nearest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NO_TRI = 0xFFFFFFFF
FLT_MAX = F(3.40282347e+38)
EMPTY_REF, LEAF_BIT, FIRST_MASK = 0xFFFFFFFF, 0x80000000, 0x07FFFFFF
START, FACE, E01, E02, E12, V0, V1, V2 = range(8)  # which candidate gave t (tri_sweep's debug return); -1: none
SHIFT = F([1000, -2000, 500])

SNIPPET = r"""
#include <cstddef>
#include <beam/Beam.h>
static_assert(sizeof(bm_sweep) == 32 && sizeof(bm_sweep) == sizeof(bm_ray), "record size");
static_assert(offsetof(bm_sweep, origin) == 0 && offsetof(bm_sweep, tmax) == 12 && offsetof(bm_sweep, dir) == 16 &&
              offsetof(bm_sweep, radius) == 28 && offsetof(bm_ray, pad) == 28, "bm_sweep is bm_ray with pad = radius");
static_assert(BM_SWEEP_CLOSEST == 0u && BM_SWEEP_ANY == 1u, "constants");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    return (int)scene->sweepSpheres(nullptr, 0, BM_SWEEP_CLOSEST, nullptr);
}
"""


# ---- the restatement ---------------------------------------------------------------------------------
def _dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z of two component triples."""
    x = a[0] * b[0]
    y = a[1] * b[1]
    s = x + y
    z = a[2] * b[2]
    return s + z


def _cross(x, y):
    """(x.y*y.z - y.y*x.z, x.z*y.x - y.z*x.x, x.x*y.y - y.x*x.y)."""
    out = []
    for i, j in ((1, 2), (2, 0), (0, 1)):
        a = x[i] * y[j]
        b = y[i] * x[j]
        out.append(a - b)
    return out


def _sub(a, b):
    return [a[k] - b[k] for k in range(3)]


def _edge(m, E, d, dd, md, mm, rr, tl, zero, one):
    EE = _dot(E, E)
    Ed = _dot(E, d)
    Em = _dot(E, m)
    a = EE * dd
    b = Ed * Ed
    qa = a - b
    a = EE * md
    b = Ed * Em
    qb = a - b
    a = mm - rr
    a = EE * a
    b = Em * Em
    qc = a - b
    a = qb * qb
    b = qa * qc
    disc = a - b
    sq = np.sqrt(disc)
    num = -qb - sq
    t = num / qa
    a = t * Ed
    a = Em + a
    s = a / EE
    ok = (disc >= zero) & (qa > zero) & (s >= zero) & (s <= one) & (t >= zero) & (t <= tl)
    return ok, t, s


def _vertex(dd, md, mm, rr, tl, zero):
    a = md * md
    b = mm - rr
    b = dd * b
    disc = a - b
    sq = np.sqrt(disc)
    num = -md - sq
    t = num / dd
    ok = (disc >= zero) & (dd > zero) & (t >= zero) & (t <= tl)
    return ok, t


def tri_sweep(o, d, r, tmax, v0, v1, v2, dtype=F):
    """The header's swept-sphere function for sweeps (o, d (..., 3), r, tmax (...)) against triangles v0, v1, v2
    (..., 3), broadcast against each other: (accepted, t, u, v, kind) in `dtype`, one rounding per statement.
    kind: START, FACE, E01, E02, E12, V0, V1, V2, or -1 where nothing is accepted (t is then +inf)."""
    T = dtype
    o, d, v0, v1, v2 = (np.asarray(a, F).astype(T) for a in (o, d, v0, v1, v2))
    r, tmax = np.asarray(r, F).astype(T), np.asarray(tmax, F).astype(T)
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        dd0, u0, vv0, _ = tri_nearest(o, v0, v1, v2, T)
        tl = np.minimum(tmax, T(FLT_MAX))
        rr = r * r
        e1 = [v1[..., k] - v0[..., k] for k in range(3)]
        e2 = [v2[..., k] - v0[..., k] for k in range(3)]
        ap = [o[..., k] - v0[..., k] for k in range(3)]
        dv = [d[..., k] for k in range(3)]
        dd = _dot(dv, dv)
        # 1. the face
        n = _cross(e1, e2)
        nn = _dot(n, n)
        h = _dot(n, ap)
        nd = _dot(n, dv)
        ln = np.sqrt(nn)
        hs = np.abs(h)
        nds = np.where(h >= zero, nd, -nd)
        a = r * ln
        num = hs - a
        tf = num / (-nds)
        w = []
        for k in range(3):
            a = dv[k] * tf
            w.append(ap[k] + a)
        a = _dot(n, _cross(w, e2))
        fu = a / nn
        a = _dot(n, _cross(e1, w))
        fv = a / nn
        fs = fu + fv
        ok = (nds < zero) & (fu >= zero) & (fv >= zero) & (fs <= one) & (tf >= zero) & (tf <= tl)
        shape = np.broadcast(dd0, tf).shape
        tb = np.full(shape, np.inf, T)
        ub, vb = np.zeros(shape, T), np.zeros(shape, T)
        kind = np.full(shape, -1, np.int8)

        def take(ok, t, u, v, k):
            sel = ok & (t < tb)  # strict: the earlier candidate keeps an equal t
            tb[sel] = np.broadcast_to(t, shape)[sel]
            ub[sel] = np.broadcast_to(u, shape)[sel]
            vb[sel] = np.broadcast_to(v, shape)[sel]
            kind[sel] = k

        take(ok, tf, fu, fv, FACE)
        md0 = _dot(ap, dv)
        mm0 = _dot(ap, ap)
        m1 = _sub(ap, e1)
        m2 = _sub(ap, e2)
        md1 = _dot(m1, dv)
        mm1 = _dot(m1, m1)
        md2 = _dot(m2, dv)
        mm2 = _dot(m2, m2)
        ok, t, s = _edge(ap, e1, dv, dd, md0, mm0, rr, tl, zero, one)
        take(ok, t, s, zero, E01)
        ok, t, s = _edge(ap, e2, dv, dd, md0, mm0, rr, tl, zero, one)
        take(ok, t, zero, s, E02)
        ok, t, s = _edge(m1, _sub(e2, e1), dv, dd, md1, mm1, rr, tl, zero, one)
        take(ok, t, one - s, s, E12)
        ok, t = _vertex(dd, md0, mm0, rr, tl, zero)
        take(ok, t, zero, zero, V0)
        ok, t = _vertex(dd, md1, mm1, rr, tl, zero)
        take(ok, t, one, zero, V1)
        ok, t = _vertex(dd, md2, mm2, rr, tl, zero)
        take(ok, t, zero, one, V2)
        start = np.broadcast_to(dd0 <= rr, shape)  # false for NaN
        tb[start] = zero
        ub[start] = np.broadcast_to(u0, shape)[start]
        vb[start] = np.broadcast_to(vv0, shape)[start]
        kind[start] = START
    return kind >= 0, tb, ub, vb, kind


def valid_sweeps(o, d, r, tmax):
    with np.errstate(all="ignore"):
        return (np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1) & (tmax >= 0) &
                (r > 0) & (r < np.inf))


def brute_force_sweep(origins, dirs, radii, tmax, verts, pairs=1 << 20):
    """The records bm_scene_sweep_spheres must write in BM_SWEEP_CLOSEST mode for the sweeps (origins, dirs (n,3),
    radii, tmax: scalars or (n,)) over the triangles verts (ntri,3,3) in global-id order: {"t","u","v","tri_id",
    "kind"}, and "any": BM_SWEEP_ANY's byte. Every triangle is evaluated for every valid sweep."""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(dirs, F).reshape(-1, 3)
    n, ntri = o.shape[0], verts.shape[0]
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, F), (n,)))
    tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F), (n,)))
    out = {"t": np.full(n, np.inf, F), "u": np.zeros(n, F), "v": np.zeros(n, F),
           "tri_id": np.full(n, NO_TRI, np.uint32), "kind": np.full(n, -1, np.int8), "any": np.zeros(n, np.uint8)}
    idx = np.flatnonzero(valid_sweeps(o, d, r, tm))
    if ntri == 0 or idx.size == 0:
        return out
    v0, v1, v2 = (np.ascontiguousarray(verts[None, :, k, :], F) for k in range(3))
    step = max(1, pairs // ntri)

    def chunk(at):
        sel = idx[at:at + step]
        acc, t, u, v, kind = tri_sweep(o[sel, None, :], d[sel, None, :], r[sel, None], tm[sel, None], v0, v1, v2)
        g = np.argmin(t, axis=1)  # t is +inf where nothing is accepted; the first minimum: the lowest id
        rows = np.arange(sel.size)
        won = acc[rows, g]
        w, gw, rw = sel[won], g[won], rows[won]
        return w, gw, t[rw, gw], u[rw, gw], v[rw, gw], kind[rw, gw]

    # the chunks are independent and numpy releases the interpreter lock inside its loops
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        for w, gw, t, u, v, kind in pool.map(chunk, range(0, idx.size, step)):
            out["t"][w], out["u"][w], out["v"][w] = t, u, v
            out["tri_id"][w], out["kind"][w], out["any"][w] = gw, kind, 1
    return out


# ---- the kernel's pruning margin, restated (bm_sweep_dev.h sweep_margin, k_sweep_spheres) ----------------
def sweep_margin(o, r, lo, hi):
    """m of sweeps with origins o (n,3) and radii r (n,) over a scene whose root boxes span lo..hi (float32)."""
    o, r, lo, hi = np.asarray(o, F), np.asarray(r, F), np.asarray(lo, F), np.asarray(hi, F)
    rel = np.maximum(np.abs(o - lo), np.abs(hi - o)).max(axis=1)
    root = np.maximum(np.abs(lo), np.abs(hi)).max()
    big = np.abs(o).max(axis=1) + root
    a = F(2.0 ** -7) * (rel + r)
    b = F(2.0 ** -16) * big
    return a + b


def bounds(verts):
    p = np.asarray(verts, F).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def tri_vertices(meshes):
    return np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes] + [np.zeros((0, 3, 3), F)])


def translated(meshes, shift):
    return [dict(m, pos=np.asarray(m["pos"], F).reshape(-1, 3) + F(shift)) for m in meshes]


# ---- the sample ----------------------------------------------------------------------------------------
def make_sweeps(verts, n, seed, radii=(0.002, 0.3), bounded_every=5):
    """n sweeps at the triangles verts: origins 0.2-2 box diagonals from the centre, directions towards random
    points of the box (not normalised: t = 1 is that point), radii log-uniform in radii x the diagonal, tmax
    +inf but for every bounded_every-th sweep (0.3-1.5). Returns (o, d, r, tmax) in float32."""
    rng = np.random.default_rng(seed)
    lo, hi = (a.astype(np.float64) for a in bounds(verts))
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = F(c + u * rng.uniform(0.2, 2.0, (n, 1)) * diag)
    target = F(lo + rng.uniform(0, 1, (n, 3)) * (hi - lo))
    d = target - o
    r = F(diag * np.exp(rng.uniform(np.log(radii[0]), np.log(radii[1]), n)))
    tmax = np.full(n, np.inf, F)
    if bounded_every:
        tmax[::bounded_every] = F(rng.uniform(0.3, 1.5, tmax[::bounded_every].shape))
    return o, d, r, tmax


_SAMPLE = {}


def sample():
    """The three thirds of the quality and lemma tests, 300 sweeps each at the suzanne fixture: "wide" radii
    0.2-30 % of the diagonal, "thin" 1e-5-1e-4 of it, "far" the wide ones with mesh and origins translated by
    SHIFT. name -> (verts, (o, d, r, tmax), brute force). Computed once per process, read-only."""
    if not _SAMPLE:
        base = scenes.load_mesh("suzanne")
        for name, meshes, radii, seed in (("wide", base, (0.002, 0.3), 11), ("thin", base, (1e-5, 1e-4), 12),
                                          ("far", translated(base, SHIFT), (0.002, 0.3), 13)):
            verts = tri_vertices(meshes)
            sw = make_sweeps(verts, 300, seed, radii)
            exp = brute_force_sweep(*sw, verts)
            for a in list(sw) + list(exp.values()):
                a.setflags(write=False)
            _SAMPLE[name] = (verts, sw, exp)
    return _SAMPLE


# ---- float64 geometry: the distance from points to a mesh -------------------------------------------------
def _groups(centres, idx, size, out):
    if idx.size <= size:
        out.append(idx)
        return
    c = centres[idx]
    axis = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
    order = idx[np.argsort(c[:, axis], kind="stable")]
    _groups(centres, order[:idx.size // 2], size, out)
    _groups(centres, order[idx.size // 2:], size, out)


class MeshDistance:
    """dist(p, mesh) in float64: test_points_abi.tri_nearest in float64 over the triangles of every group (64
    triangles, split by medians) whose bounding sphere comes within the best distance found so far."""

    def __init__(self, verts, size=64):
        self.v = np.asarray(verts, F).astype(np.float64)
        groups = []
        _groups(self.v.mean(axis=1), np.arange(self.v.shape[0]), size, groups)
        self.groups = groups
        self.centre = np.stack([self.v[g].reshape(-1, 3).mean(axis=0) for g in groups])
        self.radius = np.array([np.linalg.norm(self.v[g].reshape(-1, 3) - c, axis=1).max()
                                for g, c in zip(groups, self.centre)])

    def _group(self, p, g):
        t = self.v[self.groups[g]]
        dd, _, _, _ = tri_nearest(p[:, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2], np.float64)
        return np.sqrt(np.nanmin(dd, axis=1))

    def __call__(self, points):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        lb = np.maximum(np.linalg.norm(p[:, None, :] - self.centre[None], axis=2) - self.radius[None], 0.0)
        best = np.full(p.shape[0], np.inf)
        first = np.argmin(lb, axis=1)
        for g in np.unique(first):  # an upper bound from each point's nearest group
            sel = np.flatnonzero(first == g)
            best[sel] = self._group(p[sel], g)
        for g in range(len(self.groups)):
            sel = np.flatnonzero((lb[:, g] <= best) & (first != g))
            if sel.size:
                best[sel] = np.minimum(best[sel], self._group(p[sel], g))
        return best


# Measured on x86-64 over sample(), in units of 2^-24 * S, S the largest |coordinate| of the origin, of c(t) and
# of the mesh (each line: the third, the figure, the asserted bound = 4 x the figure rounded up to a power of two):
#   residual dist64(c(t), mesh) - r of the hits with t > 0, largest and lowest
#   clearance: the lowest dist64(c(s), mesh) - r over 64 samples s of [0, t) (a miss: of [0, min(tmax, 4)])
QUALITY = {  # third: (residual up, residual down, clearance down), measured; the bounds follow from them
    "wide": (848.8, -244.9, 0.0),   # bounds 4096, 1024, 1
    "thin": (9161.2, -2.8, 0.0),    # bounds 65536, 16, 1: mm - rr cancels, the discriminant's error is what remains
    "far": (0.5, -1.3, 0.0),        # bounds 2, 8, 1: S is 2000 here, the unit 400 times the other thirds'

}


def bound_of(measured):
    """Four times the measured figure, rounded up to a power of two (at least 1 unit)."""
    return float(2.0 ** np.ceil(np.log2(max(4.0 * abs(measured), 1.0))))


def test_quality_against_float64_geometry():
    hits = starts = total = 0
    for name, (verts, (o, d, r, tmax), exp) in sample().items():
        dist = MeshDistance(verts)
        o64, d64, r64 = o.astype(np.float64), d.astype(np.float64), r.astype(np.float64)
        hit = exp["tri_id"] != NO_TRI
        t = np.where(hit, exp["t"], 0).astype(np.float64)
        ct = o64 + t[:, None] * d64
        S = np.maximum(np.maximum(np.abs(o64).max(axis=1), np.abs(ct).max(axis=1)), np.abs(verts).max())
        unit = 2.0 ** -24 * S
        moving = hit & (exp["t"] > 0)
        resid = np.zeros(o.shape[0])
        resid[moving] = (dist(ct[moving]) - r64[moving]) / unit[moving]
        # clearance on the way: 64 samples of [0, t), for a miss of [0, min(tmax, 4)]
        end = np.where(hit, t, np.minimum(tmax.astype(np.float64), 4.0))
        s = end[:, None] * (np.arange(64) / 64.0)[None, :]
        pts = o64[:, None, :] + s[:, :, None] * d64[:, None, :]
        clear = (dist(pts.reshape(-1, 3)).reshape(-1, 64) - r64[:, None]).min(axis=1) / unit
        clear[hit & ~moving] = 0.0  # a start has no way
        up, down, cdown = resid.max(), resid.min(), clear.min()
        m = sweep_margin(o, r, *bounds(verts)).astype(np.float64)
        slack = (m / np.maximum(4.0 * np.maximum(resid, 0.0) * unit, 1e-300)).min()
        print(f"{name}: {int(hit.sum())} hits, {int((hit & ~moving).sum())} starts of {o.shape[0]}; residual "
              f"{down:+.1f} .. {up:+.1f}, lowest clearance {cdown:+.1f} (units of 2^-24 S); smallest m / (4 x upward "
              f"residual) {slack:.2f}")
        mu, md, mc = QUALITY[name]
        assert up <= bound_of(mu), (name, up)
        assert down >= -bound_of(md), (name, down)
        assert cdown >= -bound_of(mc), (name, cdown)
        assert (4.0 * np.maximum(resid, 0.0) * unit < m).all(), name  # the pruning margin covers it four times
        hits, starts, total = hits + int(hit.sum()), starts + int((hit & ~moving).sum()), total + o.shape[0]
    assert hits >= 0.40 * total and starts >= 0.01 * total, (hits, starts, total)


# ---- which candidate wins ------------------------------------------------------------------------------
COVER_TRI = F([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]])
COVER_R = F(0.25)
COVER = [  # (origin, dir, the candidate that wins)
    ((0.5, 0.5, 0.125), (0, 0, -1), START),
    ((0.5, 0.5, 2.0), (0, 0, -1), FACE),
    ((1.0, -1.0, 0.0), (0, 1, 0), E01),
    ((-1.0, 1.0, 0.0), (1, 0, 0), E02),
    ((2.0, 2.0, 0.0), (-1, -1, 0), E12),
    ((-1.0, -1.0, 0.5), (1, 1, -0.5), V0),
    ((4.0, -1.0, 0.5), (-2, 1, -0.5), V1),
    ((-1.0, 4.0, 0.5), (1, -2, -0.5), V2),
]


def cover_sweeps():
    o = F([c[0] for c in COVER])
    d = F([c[1] for c in COVER])
    return o, d, np.full(len(COVER), COVER_R, F), np.full(len(COVER), np.inf, F)


def test_every_candidate_wins_somewhere():
    o, d, r, tmax = cover_sweeps()
    exp = brute_force_sweep(o, d, r, tmax, COVER_TRI)
    assert exp["kind"].tolist() == [c[2] for c in COVER], exp["kind"].tolist()
    assert (exp["tri_id"] == 0).all() and exp["t"][0] == 0 and (exp["t"][1:] > 0).all()
    assert exp["t"][1] == F(1.75) and exp["t"][2] == F(0.75) and exp["t"][3] == F(0.75)
    # the contact point lies at distance r from the centre, in float64, for every kind
    v0, v1, v2 = COVER_TRI[0].astype(np.float64)
    u, v = exp["u"].astype(np.float64)[:, None], exp["v"].astype(np.float64)[:, None]
    contact = v0 * (1 - (u + v)) + v1 * u + v2 * v
    centre = o.astype(np.float64) + exp["t"].astype(np.float64)[:, None] * d.astype(np.float64)
    gap = np.linalg.norm(centre - contact, axis=1)
    assert (np.abs(gap[1:] - COVER_R) < 1e-5).all(), gap
    assert gap[0] < COVER_R


def test_brute_force_rules():
    """Ties go to the lowest id, tmax bounds by t <= tmax and is honoured by the any byte, tmax = 0 asks about the
    start alone, invalid sweeps get the miss record."""
    tri = COVER_TRI[0]
    verts = np.stack([tri + F([0, 0, -1]), tri, tri])
    o, d = F([[0.5, 0.5, 2.0]] * 6), F([[0, 0, -1]] * 6)
    tmax = F([np.inf, 1.75, np.nextafter(F(1.75), F(0)), 0.0, -1.0, np.nan])
    exp = brute_force_sweep(o, d, COVER_R, tmax, verts)
    assert exp["tri_id"].tolist() == [1, 1, NO_TRI, NO_TRI, NO_TRI, NO_TRI]
    assert exp["any"].tolist() == [1, 1, 0, 0, 0, 0] and exp["t"][1] == F(1.75)
    start = brute_force_sweep(F([[0.5, 0.5, 0.2]]), F([[0, 0, 1]]), COVER_R, F(0.0), verts)
    assert start["tri_id"].tolist() == [1] and start["t"][0] == 0 and start["kind"][0] == START
    bad = brute_force_sweep(F([[0.5, 0.5, 2.0]] * 6), F([[0, 0, -1], [0, 0, 0], [np.nan, 0, -1], [0, 0, -1], [0, 0, -1],
                                                         [0, 0, -1]]),
                            F([0.25, 0.25, 0.25, 0.0, -1.0, np.inf]), np.inf, verts)
    assert bad["tri_id"].tolist() == [1] + [NO_TRI] * 5 and np.isposinf(bad["t"][1:]).all()
    assert bad["any"].tolist() == [1, 0, 0, 0, 0, 0]


# ---- the traversal loses nothing: the node test walked over the oracle's BVH4 ---------------------------
def walk(rec, tris, verts, o, d, r, tmax, pad, bound):
    """The kernel's node test in numpy over exported BVH4 records (n, 32) and triangle records (ntri, 12): a
    child is kept when ref != EMPTY_REF and the centre's line o + t d meets its box moved outwards by pad with
    tn <= tf, tf >= 0 and tn <= bound — bound being the final t, the tightest the kernel's bound ever gets, so
    the kernel keeps at least these children. Returns the (t, id)-minimum tri_sweep accepts among the leaves
    reached as (t, u, v, id) and the number of leaf triangles evaluated."""
    box = rec[:, :24].view(F).reshape(-1, 6, 4)
    ref = rec[:, 24:28]
    reached = []
    front = np.zeros(1 if tris.shape[0] else 0, np.int64)
    with np.errstate(all="ignore"):
        inv = F(1) / d
        while front.size:
            b, rf = box[front], ref[front]  # (m, 6, 4), (m, 4)
            tn = np.full(rf.shape, -np.inf, F)
            tf = np.full(rf.shape, np.inf, F)
            for a in range(3):
                lo = b[:, a, :] - pad
                hi = b[:, 3 + a, :] + pad
                t0 = (lo - o[a]) * inv[a]
                t1 = (hi - o[a]) * inv[a]
                tn = np.fmax(tn, np.fmin(t0, t1))
                tf = np.fmin(tf, np.fmax(t0, t1))
            keep = (rf != EMPTY_REF) & (tn <= tf) & (tf >= 0) & (tn <= bound)
            kept = rf[keep]
            front = kept[(kept & LEAF_BIT) == 0].astype(np.int64)
            for lf in kept[(kept & LEAF_BIT) != 0]:
                first, cnt = int(lf & FIRST_MASK), int((lf >> 27) & 15) + 1
                reached.append(tris[first:first + cnt, 3])
    if not reached:
        return (F(np.inf), F(0), F(0), NO_TRI), 0
    ids = np.sort(np.concatenate(reached))
    # by global id from the brute force's vertices (check_walk asserts that the records hold the same edges)
    acc, tt, uu, vv, _ = tri_sweep(o, d, r, tmax, verts[ids, 0], verts[ids, 1], verts[ids, 2])
    j = int(np.argmin(tt))  # +inf where nothing is accepted; ids ascend: the first minimum is the lowest id
    if not acc[j]:
        return (F(np.inf), F(0), F(0), NO_TRI), ids.size
    return (tt[j], uu[j], vv[j], int(ids[j])), ids.size


def check_walk(oracle, meshes, verts, sweeps, exp, name, every=1):
    rec, tris, _, _ = oracle.bvh_build(meshes, 4, width=4).export()
    assert rec.shape[1] == 32 and tris.shape[0] == verts.shape[0]
    # the record's edges are the brute force's (the same two subtractions)
    tf32, gid = tris.view(F), tris[:, 3]
    assert np.array_equal(tf32[:, 0:3], verts[gid, 0]) and np.array_equal(tf32[:, 4:7], verts[gid, 1] - verts[gid, 0])
    assert np.array_equal(tf32[:, 8:11], verts[gid, 2] - verts[gid, 0])
    # the margin's scale: the union of the root record's child boxes is the mesh's bounding box, or holds it
    box = rec[0, :24].view(F).reshape(6, 4)
    lo, hi = np.fmin.reduce(box[0:3], axis=1), np.fmax.reduce(box[3:6], axis=1)
    mlo, mhi = bounds(verts)
    assert (lo <= mlo).all() and (hi >= mhi).all()
    o, d, r, tmax = sweeps
    pad = r + sweep_margin(o, r, lo, hi)
    tested = hits = 0
    for i in range(0, o.shape[0], every):
        if exp["tri_id"][i] == NO_TRI:
            continue
        (t, u, v, g), n = walk(rec, tris, verts, o[i], d[i], r[i], tmax[i], pad[i], exp["t"][i])
        tested, hits = tested + n, hits + 1
        assert g == exp["tri_id"][i] and t == exp["t"][i], (name, i, t, g, exp["t"][i], exp["tri_id"][i])
        assert F(u).view(np.uint32) == exp["u"][i].view(np.uint32) and F(v).view(np.uint32) == exp["v"][i].view(np.uint32)
    return tested, hits


def deep_sweeps(n=48):
    """Sweeps through the deep chain of tests/deep_scenes.py: its query origins, towards points of the chain's
    box, with a radius that meets the sibling boxes."""
    import deep_scenes
    o, d = deep_scenes.ray_batch(n)
    return o, d, np.full(n, 64.0, F), np.full(n, np.inf, F)


def test_the_node_test_loses_no_accepted_contact(oracle):
    import deep_scenes
    base = scenes.load_mesh("suzanne")
    for name, (verts, sw, exp) in sample().items():
        meshes = translated(base, SHIFT) if name == "far" else base
        tested, hits = check_walk(oracle, meshes, verts, sw, exp, name)
        assert hits >= 100, (name, hits)
        print(f"{name}: {hits} hits walked, {tested / hits:.0f} of {verts.shape[0]} triangles evaluated per sweep")
        if name == "wide":
            assert tested < 0.25 * hits * verts.shape[0]  # and it does prune
    meshes = deep_scenes.deep_meshes()
    verts = tri_vertices(meshes)
    sw = deep_sweeps()
    exp = brute_force_sweep(*sw, verts)
    tested, hits = check_walk(oracle, meshes, verts, sw, exp, "deep")
    assert hits >= 24, hits


# ---- the ABI -------------------------------------------------------------------------------------------
def test_record_layout_and_constants():
    assert C.sizeof(_lib.Sweep) == 32 == C.sizeof(_lib.Ray)
    assert _lib.Sweep.origin.offset == 0 and _lib.Sweep.tmax.offset == 12
    assert _lib.Sweep.dir.offset == 16 and _lib.Sweep.radius.offset == 28 == _lib.Ray.pad.offset
    assert (_lib.SWEEP_CLOSEST, _lib.SWEEP_ANY) == (0, 1)
    header = open(_lib.HEADER).read()
    assert "#define BM_SWEEP_CLOSEST 0u" in header and "#define BM_SWEEP_ANY 1u" in header


def test_prototypes():
    P, U = C.c_void_p, C.c_uint32
    assert _lib.SIGNATURES["bm_scene_sweep_spheres"] == (C.c_int32, [P, P, U, U, U, P])
    assert _lib.SIGNATURES["bm_scene_sweep_spheres_counters"] == (C.c_int32, [P, P, U, U, U, P, C.POINTER(C.c_uint64)])
    assert {"bm_scene_sweep_spheres", "bm_scene_sweep_spheres_counters"} <= set(_lib.declared_symbols())


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    for mode in (_lib.SWEEP_CLOSEST, _lib.SWEEP_ANY, 2):
        assert lib.bm_scene_sweep_spheres(None, None, 0, mode, 0, None) == bad
        assert lib.bm_scene_sweep_spheres(None, None, 16, mode, 0, None) == bad
        assert lib.bm_scene_sweep_spheres_counters(None, None, 0, mode, 0, None, out) == bad
        assert lib.bm_scene_sweep_spheres_counters(None, None, 0, mode, 0, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::sweepSpheres of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "sweep.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "sweep"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()
