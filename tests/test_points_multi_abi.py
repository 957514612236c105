"""Multi-result point queries (bm_scene_closest_points_multi): the ABI's layout, null handling, the C++ layer, and
the yardstick and designed point sets the GPU tests use (CPU).

The yardstick is brute_points_multi: tests/test_points_abi.py's tri_nearest (the numpy float32 restatement of the
header's triangle function, checked there against float64) evaluated for every triangle and every valid point,
the triangles with dd <= rmax*rmax sorted by (dd, id) and the first k kept. No value in it comes from the
library. At k = 1 it must equal that module's brute_force bit for bit.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracercuda_amd import _lib, scenes
from test_points_abi import F, NO_TRI, brute_force, tri_nearest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 16
KEYS = ("t", "u", "v", "tri_id")
SIGNATURE = _lib.SIGNATURES["bm_scene_closest_points_multi"]  # the query all of this is about: no binding, no tests

SNIPPET = r"""
#include <beam/Beam.h>
static_assert(sizeof(bm_point) == 16 && sizeof(bm_hit) == 16, "record sizes");
static_assert(BM_MULTI_MAX_HITS == 16u && BM_MULTI_COUNT_ALL == 1u, "constants");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    uint32_t* counts = nullptr;
    return (int)(scene->closestPointsMulti(nullptr, 0, 4, 0, nullptr) +
                 scene->closestPointsMulti(nullptr, 0, 0, BM_MULTI_COUNT_ALL, nullptr, counts));
}
"""


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the brute force ---------------------------------------------------------------------------------
def brute_points_multi(points, rmax, verts, k, count_all=False, pairs=1 << 21):
    """The records bm_scene_closest_points_multi must write for points (n,3) with rmax (n,) or a scalar over the
    triangles verts (ntri,3,3) in global-id order: {"t","u","v","tri_id"} of shape (n, k), the first k elements
    of each point's N in (dd, id) order with t = sqrtf(dd) (miss records behind them), "dd" (n, k) the squared
    distances themselves (+inf in a miss slot), "count" (n,) what counts_dev holds (|N| with count_all,
    min(k, |N|) without) and "total" (n,) = |N| either way. Every triangle is evaluated for every valid point,
    chunked over points; of a chunk's rows only the entries up to the k-th smallest dd (ties included) are
    sorted."""
    points = np.asarray(points, F).reshape(-1, 3)
    n, ntri = points.shape[0], verts.shape[0]
    rmax = np.ascontiguousarray(np.broadcast_to(np.asarray(rmax, F), (n,)))
    out = {"t": np.full((n, k), np.inf, F), "u": np.zeros((n, k), F), "v": np.zeros((n, k), F),
           "tri_id": np.full((n, k), NO_TRI, np.uint32), "dd": np.full((n, k), np.inf, F),
           "total": np.zeros(n, np.uint32)}
    with np.errstate(all="ignore"):
        valid = np.isfinite(points).all(axis=1) & (rmax > 0)  # false for a NaN rmax
        lim = rmax * rmax
    idx = np.flatnonzero(valid)
    if ntri and idx.size:
        v0, v1, v2 = (np.ascontiguousarray(verts[None, :, j, :], F) for j in range(3))
        step = max(1, pairs // ntri)
        for at in range(0, idx.size, step):
            sel = idx[at:at + step]
            dd, u, v, _ = tri_nearest(points[sel, None, :], v0, v1, v2)
            with np.errstate(all="ignore"):
                acc = dd <= lim[sel, None]  # false for NaN
            out["total"][sel] = acc.sum(axis=1)
            if k == 0:
                continue
            masked = np.where(acc, dd, F(np.inf))
            if ntri > k:  # nothing beyond the k-th smallest dd of a row can be among its first k
                kth = np.partition(masked, k - 1, axis=1)[:, k - 1]
                near = acc & (masked <= kth[:, None])
            else:
                near = acc
            r, g = np.nonzero(near)
            da = dd[r, g]
            order = np.lexsort((g, da, r))  # by point, then dd, then id
            r, g, da = r[order], g[order], da[order]
            cnt = np.bincount(r, minlength=sel.size)
            j = np.arange(r.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # rank within the point
            keep = j < k
            rr, jj, gg = sel[r[keep]], j[keep], g[keep]
            out["dd"][rr, jj] = da[keep]
            out["t"][rr, jj] = np.sqrt(da[keep])
            out["u"][rr, jj] = u[r[keep], gg]
            out["v"][rr, jj] = v[r[keep], gg]
            out["tri_id"][rr, jj] = gg
    out["count"] = out["total"].copy() if count_all else np.minimum(out["total"], np.uint32(k))
    assert out["t"].dtype == F and out["dd"].dtype == F
    return out


def first_k(exp, k, count_all=False):
    """brute_points_multi's answer for a smaller k, from its answer `exp` for the same points and rmax."""
    assert k <= exp["t"].shape[1]
    res = {key: exp[key][:, :k] for key in KEYS + ("dd",)}
    res["total"] = exp["total"]
    res["count"] = exp["total"] if count_all else np.minimum(exp["total"], np.uint32(k))
    return res


# ---- scenes and point sets the GPU tests share -------------------------------------------------------
def tri_vertices(meshes):
    """(ntri, 3, 3) vertex positions by global triangle id (scene order, then face order)."""
    return np.concatenate([np.asarray(m["pos"], F).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                           for m in meshes] + [np.zeros((0, 3, 3), F)])


def suzanne_points(n=3904):
    """tests/test_gpu_points.py's batch for Suzanne: near-surface, in-box and far points, a third each."""
    from test_gpu_points import make_points
    return make_points(scenes.load_mesh("suzanne"), n, 7)


RADIUS_POINTS = 504  # every seventh class 72 times
RADIUS_COLUMNS = 40


def radius_subset():
    """Near-surface points of Suzanne (tests/test_gpu_points.py's make_points, near_only), evenly thinned. Points
    away from the surface are mostly nearest to a vertex or an edge, which several triangles share with one dd:
    a radius at the k-th distance then takes the rest of the run with it and |N| = k becomes rare (4 % of the
    in-box and 3 % of the far points at k = 4, by the brute force). Near the surface the nearest points lie in
    face interiors and the construction's seven classes keep about their 1/7 each."""
    from test_gpu_points import make_points
    near = make_points(scenes.load_mesh("suzanne"), 3904, 7, near_only=True)
    return near[np.arange(RADIUS_POINTS) * (near.shape[0] // RADIUS_POINTS)]


def radius_classes(k):
    """The rank j whose distance point i takes as rmax, i cycling over the list; 0: half the nearest distance."""
    return [0, 1, k - 1, k, k + 1, 17, 40]


def radius_set(sorted_dd, k):
    """rmax (n,) by construction from the brute force's sorted squared distances sorted_dd (n, >= 40): point i
    takes the j-th nearest triangle's sqrtf(dd), j = radius_classes(k)[i % 7], stepped up by nextafter until
    rmax*rmax >= dd in float32, so exactly the triangles up to that distance (ties included) lie within it;
    j = 0 takes half the nearest distance, so nothing does (a point on the surface gets rmax = 0: invalid)."""
    n = sorted_dd.shape[0]
    js = np.asarray(radius_classes(k))[np.arange(n) % 7]
    dd = sorted_dd[np.arange(n), np.maximum(js, 1) - 1]
    assert np.isfinite(dd).all()
    rmax = np.sqrt(dd)
    for _ in range(4):
        low = rmax * rmax < dd
        rmax = np.where(low, np.nextafter(rmax, F(np.inf)), rmax)
    rmax = np.where(rmax > 0, rmax, F(1e-30))  # dd = 0 (a point on a vertex): a valid rmax whose square is 0
    assert (rmax * rmax >= dd).all() and rmax.dtype == F
    return np.where(js == 0, np.sqrt(sorted_dd[:, 0]) * F(0.5), rmax).astype(F), js


TIE_POINTS, TIE_COLUMNS = 160, 18


def tie_points():
    """Every 24th of suzanne_points(): near, in-box and far points alike."""
    return suzanne_points()[np.arange(TIE_POINTS) * 24]


def check_runs(exp, copies, n1):
    """A mesh added `copies` times (ids g, g + n1, ...) has bit-equal copies: in exp's rows every run of equal dd
    that ends before the last column holds each of its triangles `copies` times, ids ascending."""
    for dd, ids in zip(exp["dd"], exp["tri_id"].astype(np.int64)):
        edges = np.flatnonzero(np.diff(dd) != 0) + 1
        for lo, hi in zip(np.concatenate([[0], edges]), edges):  # the complete runs
            run = ids[lo:hi]
            assert (np.diff(run) > 0).all() and run.size % copies == 0
            base, times = np.unique(run % n1, return_counts=True)
            assert (times == copies).all() and set(run.tolist()) == {g + c * n1 for g in base for c in range(copies)}


SHARED_EDGE = F([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]],
                 [[0, 0, 2], [1, 0, 2], [1, 1, 2]], [[0, 0, 2], [1, 1, 2], [0, 1, 2]]])
SHARED_EDGE_POINTS = F([[0.5, 0.5, 1.0], [0.25, 0.25, -0.5], [0.75, 0.75, 0.0], [2.0, 2.0, 1.0], [-1.0, -1.0, 0.5],
                        [0.5, 0.5, 0.5], [0.75, 0.25, 1.0], [0.0, 0.0, 1.0]])


# ---- the brute force against tests/test_points_abi.py's --------------------------------------------------
def assert_k1_equals(points, rmax, verts):
    one = brute_points_multi(points, rmax, verts, 1)
    ref = brute_force(points, rmax, verts)
    assert np.array_equal(one["tri_id"][:, 0], ref["tri_id"])
    for key in ("t", "u", "v"):
        assert np.array_equal(bits(one[key][:, 0]), bits(ref[key])), key
    assert np.array_equal(one["count"], (ref["tri_id"] != NO_TRI).astype(np.uint32))
    return one


def test_k1_equals_the_single_result_brute_force():
    for ntri in (2, 4, 5, 17):  # tests/test_gpu_points.py's small scenes
        rng = np.random.default_rng(200 + ntri)
        base = rng.uniform(-1, 1, (ntri, 1, 3))
        verts = F(base + rng.uniform(-0.4, 0.4, (ntri, 3, 3)))
        pts = F(rng.uniform(-2, 2, (203, 3)))
        assert_k1_equals(pts, np.inf, verts)
        assert_k1_equals(pts, F(0.8), verts)
    verts = tri_vertices(scenes.load_mesh("suzanne"))
    pts = suzanne_points()[np.arange(500) * 7]
    one = assert_k1_equals(pts, np.inf, verts)
    assert (one["tri_id"] != NO_TRI).all()
    assert_k1_equals(pts, np.where(np.arange(500) % 2 == 0, one["t"][:, 0], one["t"][:, 0] * F(0.5)), verts)
    many = brute_points_multi(pts, np.inf, verts, KMAX)
    for key in KEYS:  # a larger k only appends
        assert np.array_equal(many[key][:, :1].view(np.uint32), one[key].view(np.uint32)), key
    assert (np.diff(many["dd"], axis=1) >= 0).all() and (many["total"] == verts.shape[0]).all()
    tie = many["dd"][:, 1:] == many["dd"][:, :-1]
    assert (many["tri_id"][:, 1:][tie] > many["tri_id"][:, :-1][tie]).all()


# ---- the rules, by hand ------------------------------------------------------------------------------
def test_ties_resolve_by_id():
    tri = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    verts = np.stack([tri + F([0, 0, 1]), tri, tri, tri + F([0, 0, 3])])  # ids 1 and 2 coincide
    res = brute_points_multi(F([[0.25, 0.25, 0.5]]), np.inf, verts, 4)
    assert res["tri_id"].tolist() == [[0, 1, 2, 3]] and res["t"].tolist() == [[0.5, 0.5, 0.5, 2.5]]
    for k, ids in ((1, [0]), (2, [0, 1]), (3, [0, 1, 2])):  # the cut inside the run keeps the lowest ids
        r = brute_points_multi(F([[0.25, 0.25, 0.5]]), np.inf, verts, k)
        assert r["tri_id"].tolist() == [ids] and r["count"].tolist() == [k] and r["total"].tolist() == [4]
    rev = brute_points_multi(F([[0.25, 0.25, 0.5]]), np.inf, verts[::-1], 2)
    assert rev["tri_id"].tolist() == [[1, 2]]  # the same triangles under other ids: again the lowest of the run


def test_rmax_at_and_one_ulp_below_a_distance():
    tri = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    verts = np.stack([tri, tri + F([0, 0, 3])])
    p = F([[0.25, 0.25, 1.0]])  # 1 from id 0, 2 from id 1
    at = brute_points_multi(p, F(2.0), verts, 4, count_all=True)
    assert at["tri_id"].tolist() == [[0, 1, NO_TRI, NO_TRI]] and at["count"].tolist() == [2]
    below = brute_points_multi(p, np.nextafter(F(2.0), F(0)), verts, 4, count_all=True)
    assert below["tri_id"].tolist() == [[0, NO_TRI, NO_TRI, NO_TRI]] and below["count"].tolist() == [1]
    assert np.isposinf(below["t"][0, 1:]).all() and (bits(below["u"][0, 1:]) == 0).all()
    none = brute_points_multi(p, F(0.5), verts, 4, count_all=True)
    assert none["count"].tolist() == [0] and (none["tri_id"] == NO_TRI).all()


def test_nan_dd_is_neither_listed_nor_counted():
    verts = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]],
               [[3, 0, 0], [3, 0, 0], [5, 0, 0]],     # v1 = v0: region 3 divides 0 by 0 beside its vertex regions
               [[0, 0, 5], [1, 0, 5], [0, 1, 5]]])
    p = F([[4.5, 0.5, 0.0]])
    dd, _, _, _ = tri_nearest(p[:, None, :], verts[None, :, 0], verts[None, :, 1], verts[None, :, 2])
    assert np.isnan(dd[0, 1]) and np.isfinite(dd[0, [0, 2]]).all()
    res = brute_points_multi(p, np.inf, verts, 4, count_all=True)
    assert res["tri_id"].tolist() == [[0, 2, NO_TRI, NO_TRI]] and res["count"].tolist() == [2]
    assert brute_points_multi(p, np.inf, verts[1:2], 2, count_all=True)["count"].tolist() == [0]
    # through a vertex region the same triangle counts
    assert brute_points_multi(F([[2.0, 0.0, 0.0]]), np.inf, verts[1:2], 2)["tri_id"].tolist() == [[0, NO_TRI]]


def test_invalid_points_and_k0():
    tri = F([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    pts = F([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.2, 0.2, 1], [0.2, 0.2, 1], [0.2, 0.2, 1], [0.2, 0.2, 1]])
    rmax = F([np.inf, np.inf, np.inf, np.nan, 0.0, -1.0, np.inf])
    for count_all in (False, True):
        res = brute_points_multi(pts, rmax, tri, 3, count_all)
        assert res["count"].tolist() == [0] * 6 + [1] and (res["tri_id"][:6] == NO_TRI).all()
        assert np.isposinf(res["t"][:6]).all() and (bits(res["u"][:6]) == 0).all() and (bits(res["v"][:6]) == 0).all()
    zero = brute_points_multi(pts, rmax, tri, 0, count_all=True)
    assert zero["t"].shape == (7, 0) and zero["count"].tolist() == [0] * 6 + [1]
    empty = brute_points_multi(pts, rmax, np.zeros((0, 3, 3), F), 2, count_all=True)
    assert empty["count"].tolist() == [0] * 7 and (empty["tri_id"] == NO_TRI).all()


# ---- the designed sets -------------------------------------------------------------------------------
def test_designed_sets_have_what_the_gpu_tests_need():
    verts = tri_vertices(scenes.load_mesh("suzanne"))
    pts = radius_subset()
    ranked = brute_points_multi(pts, np.inf, verts, RADIUS_COLUMNS)
    assert np.isfinite(ranked["dd"]).all()
    for k in (4, 16):
        rmax, js = radius_set(ranked["dd"], k)
        exp = brute_points_multi(pts, rmax, verts, KMAX, count_all=True)
        tot = exp["total"].astype(np.int64)
        want = np.where(js == 0, 0, js)
        assert (tot >= want).all() and (tot[js == 0] == 0).all()  # ties only add
        share = {"|N| = 0": tot == 0, "0 < |N| < k": (tot > 0) & (tot < k), "|N| = k": tot == k, "|N| > k": tot > k,
                 "|N| > 16": tot > 16}
        print(f"k = {k}: " + ", ".join(f"{name} {m.mean():.3f}" for name, m in share.items()))
        for name, m in share.items():
            assert m.mean() >= 0.10, (k, name, float(m.mean()))
        # within rmax the list is the unbounded one's head
        for j in range(min(k, KMAX)):
            inside = tot > j
            assert np.array_equal(exp["tri_id"][inside, j], ranked["tri_id"][inside, j])
    # the tie scenes: Suzanne added 3 and 6 times; a list of k = 4, 5 or 16 entries ends inside a run of equal dd
    n1 = verts.shape[0]
    tp = tie_points()
    for copies in (3, 6):
        exp = brute_points_multi(tp, np.inf, np.concatenate([verts] * copies), TIE_COLUMNS)
        check_runs(exp, copies, n1)
        for k in (4, 5, 16):
            inside = (exp["dd"][:, k - 1] == exp["dd"][:, k]) & (exp["tri_id"][:, k - 1] < exp["tri_id"][:, k])
            print(f"{copies} copies, k = {k}: the list ends inside a run on {inside.mean():.3f} of the points")
            assert inside.mean() >= 0.5, (copies, k, float(inside.mean()))
    edge = brute_points_multi(SHARED_EDGE_POINTS, np.inf, SHARED_EDGE, 4)
    run = edge["dd"][:, 0] == edge["dd"][:, 1]
    assert run.sum() >= 4 and (edge["tri_id"][run, 0] < edge["tri_id"][run, 1]).all()  # k = 1 cuts these runs


# ---- what the build's box padding does to the pruning margin -----------------------------------------
def pad_scale():
    import re
    text = open(os.path.join(REPO, "raytracercuda_amd", "csrc", "bm_common.h")).read()
    return float.fromhex(re.search(r"PAD_SCALE = (0x1p-\d+)f", text).group(1))


def test_box_padding_exceeds_what_a_relative_margin_leaves_open():
    """Why no built scene tells the absolute margin m from the relative factor 1 + 2^-18.
    The build moves every face of every box outward by at least pad = PAD_SCALE * E, E the scene's largest
    extent. For a point p outside a box B that holds a triangle T, on every axis where p is outside by d_c the
    triangle is outside by d_c + pad or more, so dist(p, T) >= dist(p, B) + pad in exact arithmetic. A bound
    dd_last * (1 + 2^-18) can then drop a subtree with a triangle that belongs in the list (dd <= dd_last) only
    where the float32 function returns t32 with t32 * (1 + 2^-19) < t - pad, t the exact distance: the function
    must fall short by more than pad plus 2^-19 of itself. Measured here as (t64 - t32 * (1 + 2^-19)) / pad with E
    taken as the triangle's own extent, the least any scene holding it has: 0.122 over this test's 400,000 pairs
    (well-shaped triangles and slivers, half of them translated along x, points from 1e-7 to 1 off the plane),
    against the 1 a loss needs; 4.8 million pairs of the same kind, with the padding's coordinate term counted
    in, gave 0.127. Without the relative part the figure is 0.978 here and reached 1.42 there, at distances far
    above pad: the padding alone does not cover a bound with no margin at all. Near the surface the padding
    covers the function's error, far from it the relative part does. The assertion is the loss condition itself."""
    rng = np.random.default_rng(11)
    scale = pad_scale()
    assert scale == 2.0 ** -20
    worst, bare = 0.0, 0.0
    for rep in range(2):
        n = 200000
        v0 = rng.uniform(-1, 1, (n, 3))
        a = rng.normal(size=(n, 3))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = np.cross(a, rng.normal(size=(n, 3)))
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        la = rng.uniform(0.05, 2, (n, 1))
        lb = la * 10 ** rng.uniform(-4, 0, (n, 1))  # down to slivers of aspect 1e4
        v1 = v0 + a * la
        v2 = v0 + a * la * rng.uniform(-1, 2, (n, 1)) + b * lb
        if rep:  # translated along x alone: the padding across y and z stays that of the extent
            shift = rng.uniform(-1, 1, (n, 3)) * np.array([1e3, 0, 0])
            v0, v1, v2 = v0 + shift, v1 + shift, v2 + shift
        v0, v1, v2 = F(v0), F(v1), F(v2)
        e1, e2 = v1.astype(np.float64) - v0, v2.astype(np.float64) - v0
        nrm = np.cross(e1, e2)
        nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
        x, y = rng.uniform(-0.5, 1.5, (n, 1)), rng.uniform(-0.5, 1.5, (n, 1))
        h = 10 ** rng.uniform(-7, 0, (n, 1)) * rng.choice([-1, 1], (n, 1))
        p = F(v0 + e1 * x + e2 * y + nrm * h)
        dd32 = tri_nearest(p, v0, v1, v2)[0]
        dd64 = tri_nearest(p, v0, v1, v2, np.float64)[0]
        ok = np.isfinite(dd32) & np.isfinite(dd64)
        t32, t64 = np.sqrt(dd32.astype(np.float64)), np.sqrt(dd64)
        verts = np.stack([v0, v1, v2]).astype(np.float64)
        pad = scale * (verts.max(0) - verts.min(0)).max(1)
        worst = max(worst, float(((t64 - t32 * (1 + 2.0 ** -19)) / pad)[ok].max()))
        bare = max(bare, float(((t64 - t32) / pad)[ok].max()))
    print(f"box padding: largest (t64 - t32 (1 + 2^-19)) / pad = {worst:.3f}, without the relative part {bare:.3f}")
    assert worst < 1.0, worst


# ---- ABI ---------------------------------------------------------------------------------------------
def test_record_layout_and_constants():
    assert C.sizeof(_lib.Point) == 16 and C.sizeof(_lib.Hit) == 16
    assert _lib.Hit.t.offset == 0 and _lib.Hit.u.offset == 4 and _lib.Hit.v.offset == 8 and _lib.Hit.tri_id.offset == 12
    assert _lib.MULTI_MAX_HITS == 16 and _lib.MULTI_COUNT_ALL == 1
    res, args = SIGNATURE
    assert res is C.c_int32 and len(args) == 7
    assert len(_lib.SIGNATURES["bm_scene_closest_points_multi_counters"][1]) == 8
    assert {"bm_scene_closest_points_multi", "bm_scene_closest_points_multi_counters"} <= set(_lib.declared_symbols())


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    assert lib.bm_scene_closest_points_multi(None, None, 0, 4, 0, None, None) == bad
    assert lib.bm_scene_closest_points_multi(None, None, 16, 4, 0, None, None) == bad
    assert lib.bm_scene_closest_points_multi(None, None, 0, 0, _lib.MULTI_COUNT_ALL, None, None) == bad
    assert lib.bm_scene_closest_points_multi_counters(None, None, 0, 4, 0, None, None, out) == bad
    assert lib.bm_scene_closest_points_multi_counters(None, None, 0, 4, 0, None, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::closestPointsMulti of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "points_multi.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "points_multi"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()
