"""Ray query filters (BM_RAYS_CULL_*, BM_RAYS_PAD_*, entry masks): the constants, the Python packing of the pad
word, the C++ layer, and the yardstick the GPU tests compare with (CPU).

The yardstick, brute_filtered, is tests/test_multihit_abi.py's brute force with the filter include/beam_c.h
states applied to every accepted triangle: the triangle function's numpy restatement (tri_hit), its determinant
recomputed by the same statements, every triangle evaluated for every valid ray. No value in it comes from the
library.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracercuda_amd import _lib, beam, scenes
from test_multihit_abi import (F, FLT_MAX, NO_TRI, bits, brute_multi, cross3, dot3, layers_mesh, layers_rays, make_batch,
                               tri_hit, tri_vertices)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACK, FRONT = _lib.RAYS_CULL_BACK, _lib.RAYS_CULL_FRONT
SKIP, TMIN, MASK = _lib.RAYS_PAD_SKIP_TRI, _lib.RAYS_PAD_TMIN, _lib.RAYS_PAD_MASK
ALL_ONES = 0xFFFFFFFF

SNIPPET = r"""
#include <beam/Beam.h>
static_assert(BM_RAYS_CULL_BACK == 0x10u && BM_RAYS_CULL_FRONT == 0x20u, "cull flags");
static_assert(BM_RAYS_PAD_SKIP_TRI == 0x40u && BM_RAYS_PAD_TMIN == 0x80u && BM_RAYS_PAD_MASK == 0x100u, "pad flags");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    uint32_t m = 0;
    return (int)(scene->setEntryMask(0, 1u) + scene->getEntryMask(0, &m) +
                 scene->traceRays(nullptr, 0, nullptr, BM_RAYS_CULL_BACK | BM_RAYS_PAD_TMIN));
}
"""


def reversed_layers():
    """layers_mesh() with the winding of the odd layers reversed (432 triangles, 18 per layer): rays from below
    meet front and back faces in turn."""
    (m,) = layers_mesh()
    idx = np.asarray(m["idx"], np.uint32).reshape(-1, 3).copy()
    odd = (np.arange(idx.shape[0]) // 18) % 2 == 1
    idx[odd] = idx[odd][:, [0, 2, 1]]
    return [dict(m, idx=idx.reshape(-1))]


def tri_det_np(d, v0, v1, v2):
    """det of the triangle function, by tri_hit's statements."""
    d, v0, v1, v2 = (np.asarray(a, F) for a in (d, v0, v1, v2))
    with np.errstate(all="ignore"):
        e1 = v1 - v0
        e2 = v2 - v0
        p = cross3(d, e2)
        det = dot3(e1, p)
    assert det.dtype == F
    return det


def owner_of(g, entry_first):
    """The scene entry that owns global id g: the last entry whose first id is <= g (an entry without triangles
    shares its first id with the next one, which owns it)."""
    return np.searchsorted(np.asarray(entry_first, np.int64), g, side="right") - 1


def brute_filtered(o, d, tmax, pad, flags, verts, entry_first=(0,), entry_mask=(ALL_ONES,), k=16, pairs=1 << 21):
    """What the filtered ray queries must write for rays (o, d) (n,3), tmax (n,) or a scalar and pad words
    (n,) uint32 or a scalar, over the triangles verts (ntri,3,3) in global-id order whose entries begin at the
    ids entry_first and carry entry_mask: {"t","u","v","tri_id"} (n, k) — the first k of each ray's filtered
    accepted set in (t, id) order, column 0 being the closest-hit record — "count" (n,) = |H| and "occluded"
    (n,) uint8, the any-hit byte (its own set: tmin < t < 1, tmax not read, a ray valid whatever its tmax)."""
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    n, ntri = o.shape[0], verts.shape[0]
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F), (n,)))
    pad = np.ascontiguousarray(np.broadcast_to(np.asarray(pad, np.uint32), (n,)))
    entry_mask = np.asarray(entry_mask, np.uint32)
    out = {"t": np.full((n, k), np.inf, F), "u": np.zeros((n, k), F), "v": np.zeros((n, k), F),
           "tri_id": np.full((n, k), NO_TRI, np.uint32), "count": np.zeros(n, np.uint32),
           "occluded": np.zeros(n, np.uint8)}
    tmin = pad.view(F) if flags & TMIN else np.zeros(n, F)
    with np.errstate(all="ignore"):
        finite = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        finite &= np.isfinite(tmin) & (tmin >= 0)  # false for NaN
        valid = finite & (tmax > 0)
    idx = np.flatnonzero(finite)
    if ntri == 0 or idx.size == 0:
        return out
    v0, v1, v2 = (np.ascontiguousarray(verts[None, :, j, :], F) for j in range(3))
    gid = np.arange(ntri)
    tri_mask = entry_mask[owner_of(gid, entry_first)]
    step = max(1, pairs // ntri)
    for at in range(0, idx.size, step):
        sel = idx[at:at + step]
        t, u, v, ok = tri_hit(o[sel, None, :], d[sel, None, :], v0, v1, v2)
        det = tri_det_np(d[sel, None, :], v0, v1, v2)
        with np.errstate(all="ignore"):
            filt = t > tmin[sel, None]
            if flags & BACK:
                filt &= det > 0
            if flags & FRONT:
                filt &= det < 0
            if flags & SKIP:
                filt &= gid[None, :] != pad[sel, None]
            if flags & MASK:
                filt &= (tri_mask[None, :] & pad[sel, None]) != 0
            base = ok & (t > F(0)) & filt  # all false for a NaN t
            out["occluded"][sel] = (base & (t < F(1))).any(axis=1)
            acc = base & (t < FLT_MAX) & (t <= tmax[sel, None]) & valid[sel, None]
        r, g = np.nonzero(acc)
        ta = t[r, g]
        order = np.lexsort((g, ta, r))  # by ray, then t, then id
        r, g, ta = r[order], g[order], ta[order]
        cnt = np.bincount(r, minlength=sel.size)
        out["count"][sel] = cnt
        j = np.arange(r.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # rank within the ray
        keep = j < k
        rr, jj, gg = sel[r[keep]], j[keep], g[keep]
        out["t"][rr, jj] = ta[keep]
        out["u"][rr, jj] = u[r[keep], gg]
        out["v"][rr, jj] = v[r[keep], gg]
        out["tri_id"][rr, jj] = gg
    return out


FIXTURES = {}


def fixture(name):
    """(verts, o, d) of the facing fixtures: the reversed layer stack with layers_rays(500), Suzanne with make_batch."""
    if name not in FIXTURES:
        if name == "layers":
            meshes = reversed_layers()
            o, d = layers_rays(500)
        else:
            meshes = scenes.load_mesh("suzanne")
            o, d = make_batch(meshes)
        FIXTURES[name] = (meshes, tri_vertices(meshes), o, d)
    return FIXTURES[name]


# ---- the yardstick's own checks ----------------------------------------------------------------------
def test_front_and_back_partition_the_accepted_set():
    for name in ("layers", "suzanne"):
        _, verts, o, d = fixture(name)
        k = 32  # every accepted triangle of every ray: 24 layers, at most 8 crossings of Suzanne
        both = brute_filtered(o, d, np.inf, 0, 0, verts, k=k)
        front = brute_filtered(o, d, np.inf, 0, BACK, verts, k=k)
        back = brute_filtered(o, d, np.inf, 0, FRONT, verts, k=k)
        assert int(both["count"].max()) <= k
        assert np.array_equal(front["count"] + back["count"], both["count"])
        assert front["count"].sum() > 0 and back["count"].sum() > 0
        for i in range(o.shape[0]):
            f = set(front["tri_id"][i, :front["count"][i]].tolist())
            b = set(back["tri_id"][i, :back["count"][i]].tolist())
            assert not (f & b) and (f | b) == set(both["tri_id"][i, :both["count"][i]].tolist())
        assert np.array_equal(both["occluded"], front["occluded"] | back["occluded"])
    # the layer stack: a ray from below sees the even layers' fronts... or backs, alternating either way
    _, verts, o, d = fixture("layers")
    front = brute_filtered(o, d, np.inf, 0, BACK, verts, k=16)
    assert np.all(front["count"] == 12) and np.all((front["tri_id"][:, :12] // 18) % 2 == (front["tri_id"][:, :1] // 18) % 2)


def test_no_reject_filters_reproduce_brute_multi():
    for name in ("layers", "suzanne"):
        _, verts, o, d = fixture(name)
        exp = brute_multi(o, d, np.inf, verts, 16)
        for flags, pad in ((0, 123), (SKIP, NO_TRI), (SKIP, verts.shape[0] + 5), (TMIN, bits(F(0.0))), (MASK, ALL_ONES)):
            got = brute_filtered(o, d, np.inf, pad, flags, verts, k=16)
            for key in ("t", "u", "v", "tri_id", "count"):
                assert np.array_equal(got[key].view(np.uint32), exp[key].view(np.uint32)), (name, flags, key)


def test_filter_rules():
    tri = F([[0, 0, 1], [1, 0, 1], [0, 1, 1]])  # cross(e1, e2) = +z: a ray along +z runs along it, a back face
    verts = np.stack([tri, tri, tri[[0, 2, 1]] + F([0, 0, 1])])  # ids 0, 1 coincide at z = 1; id 2 at z = 2 faces -z
    o, d = F([[0.25, 0.25, 0.0]]), F([[0, 0, 1]])
    assert brute_filtered(o, d, np.inf, 0, FRONT, verts, k=4)["tri_id"].tolist() == [[0, 1, NO_TRI, NO_TRI]]
    assert brute_filtered(o, d, np.inf, 0, BACK, verts, k=4)["tri_id"].tolist() == [[2, NO_TRI, NO_TRI, NO_TRI]]
    # skipping 0 returns its twin at the same t
    r = brute_filtered(o, d, np.inf, 0, SKIP, verts, k=4)
    assert r["tri_id"].tolist() == [[1, 2, NO_TRI, NO_TRI]] and r["t"][0, 0] == F(1.0) and r["count"].tolist() == [2]
    # tmin is strict; tmin >= tmax misses; an invalid tmin is an invalid ray
    assert brute_filtered(o, d, np.inf, bits(F(1.0)), TMIN, verts, k=4)["tri_id"][0, 0] == 2
    assert brute_filtered(o, d, np.inf, bits(np.nextafter(F(1.0), F(0))), TMIN, verts, k=4)["tri_id"][0, 0] == 0
    assert brute_filtered(o, d, F(1.5), bits(F(1.5)), TMIN, verts, k=4)["count"].tolist() == [0]
    for bad in (np.nan, -1.0, np.inf):
        r = brute_filtered(o, d * F(4), np.inf, bits(F(bad)), TMIN, verts, k=2)
        assert r["count"].tolist() == [0] and r["occluded"].tolist() == [0]
    assert brute_filtered(o, d * F(4), np.inf, bits(F(0.3)), TMIN, verts, k=2)["occluded"].tolist() == [1]
    assert brute_filtered(o, d * F(1.5), np.inf, bits(F(0.7)), TMIN, verts, k=2)["occluded"].tolist() == [0]
    # masks: entries [0,1) [1,2) [2,3) with masks 1, 2, 4; an entry without triangles in between owns nothing
    first, mask = (0, 1, 1, 2), (1, 8, 2, 4)
    assert owner_of(np.arange(3), first).tolist() == [0, 2, 3]
    for pad, want in ((0, []), (1, [0]), (2, [1]), (4, [2]), (8, []), (5, [0, 2]), (7, [0, 1, 2])):
        r = brute_filtered(o, d, np.inf, pad, MASK, verts, first, mask, k=4)
        assert r["tri_id"][0, :r["count"][0]].tolist() == want and r["count"][0] == len(want)


# ---- constants and packing ---------------------------------------------------------------------------
def test_constants_avoid_the_bits_existing_tests_reject():
    flags = (BACK, FRONT, SKIP, TMIN, MASK)
    assert flags == (0x10, 0x20, 0x40, 0x80, 0x100)
    for f in flags:
        assert f & (1 | 2 | 0x80000000) == 0 and f & _lib.MULTI_COUNT_ALL == 0
    header = open(_lib.HEADER).read()
    for name, val in (("CULL_BACK", "0x10u"), ("CULL_FRONT", "0x20u"), ("PAD_SKIP_TRI", "0x40u"), ("PAD_TMIN", "0x80u"),
                      ("PAD_MASK", "0x100u")):
        assert f"#define BM_RAYS_{name} {val}" in header
    assert _lib.SIGNATURES["bm_scene_set_entry_mask"][1] == [C.c_void_p, C.c_uint32, C.c_uint32]
    assert len(_lib.SIGNATURES["bm_scene_get_entry_mask"][1]) == 3


def test_pad_packing_is_bit_exact():
    n = 5
    ids = np.array([0, 7, 431, -1, 2 ** 32 - 1], np.int64)
    assert beam.ray_pad_words(n, skip_tri=ids).tolist() == [0, 7, 431, NO_TRI, NO_TRI]
    assert beam.ray_pad_words(n, skip_tri=np.int32([-1] * n)).tolist() == [NO_TRI] * n
    assert beam.ray_pad_words(n, skip_tri=np.uint32([NO_TRI] * n)).tolist() == [NO_TRI] * n
    assert beam.ray_pad_words(n, skip_tri=3).tolist() == [3] * n
    tm = F([0.0, -0.0, 1.5, np.inf, np.nan])
    assert np.array_equal(beam.ray_pad_words(n, tmin=tm), tm.view(np.uint32))
    assert beam.ray_pad_words(n, tmin=0.25).tolist() == [0x3E800000] * n
    assert beam.ray_pad_words(n, tmin=np.float64(1e-3)).tolist() == [int(F(1e-3).view(np.uint32))] * n
    assert beam.ray_pad_words(n, ray_mask=ALL_ONES).tolist() == [ALL_ONES] * n
    assert beam.ray_pad_words(n, ray_mask=np.arange(n)).tolist() == list(range(n))
    assert beam.ray_pad_words(n) is None
    assert beam.ray_filter_flags() == 0 and beam.ray_filter_flags(cull="back", tmin=0.0) == BACK | TMIN
    assert beam.ray_filter_flags(cull="front", skip_tri=1) == FRONT | SKIP and beam.ray_filter_flags(ray_mask=1) == MASK
    for kw in ({"skip_tri": 1, "tmin": 0.0}, {"tmin": 0.0, "ray_mask": 1}, {"cull": "both"}):
        try:
            beam.ray_filter_flags(**kw)
        except beam.BeamError as e:
            assert e.code == _lib.ERROR_INVALID_PARAMETER
        else:
            raise AssertionError(kw)
    # what the wrappers write: column 7 of the packed record, as the float32 view holds it
    packed = np.zeros((n, 8), F)
    packed.view(np.uint32)[:, 7] = beam.ray_pad_words(n, skip_tri=ids)
    assert _lib.Ray.pad.offset == 28 and packed.view(np.uint32)[:, 7].tolist() == [0, 7, 431, NO_TRI, NO_TRI]


def test_null_scene_without_a_device():
    lib = _lib.load()
    bad = _lib.ERROR_INVALID_PARAMETER
    m = C.c_uint32(0)
    assert lib.bm_scene_set_entry_mask(None, 0, 1) == bad
    assert lib.bm_scene_get_entry_mask(None, 0, C.byref(m)) == bad
    assert lib.bm_scene_trace_rays(None, None, 0, 0, BACK, None) == bad
    assert lib.bm_scene_trace_rays_multi(None, None, 0, 4, MASK | _lib.MULTI_COUNT_ALL, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    src = tmp_path / "filters.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "filters"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()
