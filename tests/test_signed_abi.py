"""Signed-distance and occupancy queries (bm_scene_signed_distances): why the sample directions are what they
are, the brute force, its rules, the ABI's constants, prototypes and null handling, the C++ layer (CPU).

The yardstick is brute_force_signed: the crossing count of the ray (p, D_j, +inf) is test_multihit_abi.tri_hit
(the header's ray/triangle function in numpy float32) evaluated for every triangle with the multi-hit query's
acceptance 0 < t < FLT_MAX, its parity the vote; the record is test_points_abi.brute_force's with the sign bit
of t set inside. No value in it comes from the library.
"""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from raytracercuda_amd import _lib
from test_multihit_abi import tri_hit
from test_points_abi import brute_force, tri_nearest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NO_TRI = 0xFFFFFFFF
FLT_MAX = np.finfo(np.float32).max
# the header's constants, from the decimals it quotes: the float32 values nearest to them
DA, DB, DC = F(0.80901694), F(0.309017), F(0.2317616)
DIRS = np.array([[DA, DB, DC], [-DB, DC, DA], [DC, -DA, DB]], F)

SNIPPET = r"""
#include <cstddef>
#include <beam/Beam.h>
static_assert(sizeof(bm_point) == 16 && sizeof(bm_hit) == 16, "record sizes");
static_assert(BM_SIGNED_DISTANCE == 0u && BM_SIGNED_OCCUPANCY == 1u && BM_SIGNED_VOTE3 == 1u, "constants");
static_assert(BM_SIGNED_DA == 0.80901694f && BM_SIGNED_DB == 0.309017f && BM_SIGNED_DC == 0.2317616f, "directions");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    return (int)scene->signedDistances(nullptr, 0, BM_SIGNED_DISTANCE, BM_SIGNED_VOTE3, nullptr);
}
"""


# ---- the brute force -----------------------------------------------------------------------------------
def crossing_counts(points, d, verts, pairs=1 << 21):
    """C(p) for every point (n,3): the number of triangles of verts (ntri,3,3) that tri_hit accepts for the ray
    (p, d, +inf) with 0 < t < FLT_MAX. Every triangle is evaluated for every point, chunked over points."""
    points = np.asarray(points, F).reshape(-1, 3)
    n, ntri = points.shape[0], verts.shape[0]
    out = np.zeros(n, np.uint32)
    if ntri == 0 or n == 0:
        return out
    d = np.asarray(d, F).reshape(1, 1, 3)
    v0, v1, v2 = (np.ascontiguousarray(verts[None, :, k, :], F) for k in range(3))
    step = max(1, pairs // ntri)
    for at in range(0, n, step):
        t, _, _, ok = tri_hit(points[at:at + step, None, :], d, v0, v1, v2)
        with np.errstate(all="ignore"):
            acc = ok & (t > F(0)) & (t < FLT_MAX)  # all false for a NaN t
        out[at:at + step] = acc.sum(axis=1)
    return out


def brute_force_signed(points, rmax, verts, distance=True, vote3=False):
    """What bm_scene_signed_distances must write for points (n,3) with rmax (n,) or a scalar over the triangles
    verts (ntri,3,3) in global-id order: "inside" and "votes" (uint8), "counts" (n,3: C_j, zero for an invalid
    point and for a direction not taken) and, in distance mode, {"t","u","v","tri_id"}: brute_force's record with
    the sign bit of t set inside. Points are independent, so slices of them are evaluated on a few threads."""
    points = np.asarray(points, F).reshape(-1, 3)
    n = points.shape[0]
    rmax = np.ascontiguousarray(np.broadcast_to(np.asarray(rmax, F), (n,)))
    with np.errstate(all="ignore"):
        valid = np.isfinite(points).all(axis=1)
        if distance:
            valid &= rmax > 0  # false for NaN
    counts = np.zeros((n, 3), np.uint32)
    rec = {"t": np.full(n, np.inf, F), "u": np.zeros(n, F), "v": np.zeros(n, F), "tri_id": np.full(n, NO_TRI, np.uint32)}

    def part(sel):
        for j in range(3 if vote3 else 1):
            counts[sel, j] = crossing_counts(points[sel], DIRS[j], verts)
        if distance:
            r = brute_force(points[sel], rmax[sel], verts)
            for k in rec:
                rec[k][sel] = r[k]

    idx = np.flatnonzero(valid)
    parts = [idx[at:at + 64] for at in range(0, idx.size, 64)]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(part, parts))
    return _signed_result(counts, rec if distance else None, vote3)


def _signed_result(counts, rec, vote3):
    votes = (counts & 1).sum(axis=1).astype(np.uint8)
    inside = (votes >= 2) if vote3 else (votes >= 1)
    out = {"inside": inside.astype(np.uint8), "votes": votes, "counts": counts}
    if rec is not None:
        t = rec["t"].copy()
        t.view(np.uint32)[inside] |= np.uint32(0x80000000)
        out.update(t=t, u=rec["u"], v=rec["v"], tri_id=rec["tri_id"])
    return out


def one_vote_of(exp3):
    """brute_force_signed(..., vote3=False) from its vote3=True answers for the same points: direction D0 alone."""
    counts = exp3["counts"].copy()
    counts[:, 1:] = 0
    rec = None
    if "t" in exp3:
        rec = {"t": np.abs(exp3["t"]), "u": exp3["u"], "v": exp3["v"], "tri_id": exp3["tri_id"]}
    return _signed_result(counts, rec, False)


def both_votes(points, rmax, verts):
    """{False: ..., True: ...}: brute_force_signed with one vote and with three, the triangles evaluated once."""
    exp3 = brute_force_signed(points, rmax, verts, vote3=True)
    return {False: one_vote_of(exp3), True: exp3}


# ---- meshes and points the GPU tests share ---------------------------------------------------------------
def cube_verts(drop_face=None):
    """The cube [-1,1]^3 as 12 triangles (ntri,3,3), two per face along the face's diagonal; drop_face 0..5
    leaves one face out (an open mesh)."""
    tris = []
    for face, (axis, s) in enumerate((a, s) for a in range(3) for s in (-1.0, 1.0)):
        if face == drop_face:
            continue
        u, v = (axis + 1) % 3, (axis + 2) % 3
        c = np.zeros((4, 3))
        c[:, axis] = s
        c[:, u] = [-1, 1, 1, -1]
        c[:, v] = [-1, -1, 1, 1]
        tris += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    return F(tris)


def octahedron_verts():
    """|x| + |y| + |z| <= 1 as 8 triangles."""
    e = np.eye(3)
    return F([[sx * e[0], sy * e[1], sz * e[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def icosphere_verts(subdivisions=2):
    """An icosahedron with unit vertices, every triangle split in four `subdivisions` times and the new
    vertices pushed onto the unit sphere: 20 * 4^s triangles (320 for two). Its faces lie beyond 0.97."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1)[:, None]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    tris = v[np.array(f)]
    for _ in range(subdivisions):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = ((x + y) / np.linalg.norm(x + y, axis=1)[:, None] for x, y in ((a, b), (b, c), (c, a)))
        tris = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return F(tris)


def grid_points():
    """The 25^3 multiples of 1/8 in [-1.5, 1.5]^3 (exact in float32)."""
    a = np.arange(-12, 13) / 8.0
    return F(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


def cube_inside(p):
    """(strictly inside, exactly on the surface) of the cube for grid points."""
    m = np.abs(p.astype(np.float64)).max(axis=1)
    return m < 1.0, m == 1.0


def octahedron_inside(p):
    s = np.abs(p.astype(np.float64)).sum(axis=1)
    return s < 1.0, s == 1.0


def shell_points(n=2000, seed=11):
    """n points in random directions with |p| in [0.2, 0.9] (the first half: inside the icosphere) and
    [1.05, 2] (outside)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = np.concatenate([rng.uniform(0.2, 0.9, n // 2), rng.uniform(1.05, 2.0, n - n // 2)])
    return F(u * r[:, None]), np.arange(n) < n // 2


# ---- 1. the directions -------------------------------------------------------------------------------------
def test_directions_are_the_headers():
    header = open(_lib.HEADER).read()
    for name, val in (("BM_SIGNED_DA", DA), ("BM_SIGNED_DB", DB), ("BM_SIGNED_DC", DC)):
        line = next(ln for ln in header.splitlines() if ln.startswith(f"#define {name} "))
        lit = line.split()[2]
        assert lit.startswith("0x") and lit.endswith("f"), line  # a hex float literal
        assert F(float.fromhex(lit[:-1])) == val and float(F(float.fromhex(lit[:-1]))) == float.fromhex(lit[:-1]), line
    assert (_lib.SIGNED_DA, _lib.SIGNED_DB, _lib.SIGNED_DC) == (float(DA), float(DB), float(DC))
    assert (DIRS != 0).all()


def test_cube_and_octahedron_grid():
    """Parity along each of D0, D1, D2 equals the analytic inside test at every grid point that is not exactly on
    the surface; along (1,0,0) and (1,1,1) it does not (rays through shared edges count both triangles)."""
    p = grid_points()
    assert p.shape[0] == 25 ** 3
    for name, verts, analytic, off_surface in (("cube", cube_verts(), cube_inside, 14087),
                                               ("octahedron", octahedron_verts(), octahedron_inside, 15367)):
        inside, on = analytic(p)
        keep = ~on
        assert int(keep.sum()) == off_surface and inside[keep].sum() > 100
        for j in range(3):
            par = (crossing_counts(p, DIRS[j], verts) & 1).astype(bool)
            wrong = int((par != inside)[keep].sum())
            assert wrong == 0, f"{name}: D{j} gets {wrong} of {off_surface} points wrong"
        bad = {}
        for d in ((1, 0, 0), (1, 1, 1)):
            par = (crossing_counts(p, F(d), verts) & 1).astype(bool)
            bad[d] = int((par != inside)[keep].sum())
        print(f"{name}: wrong parity at {bad[(1, 0, 0)]} (1,0,0) and {bad[(1, 1, 1)]} (1,1,1) of {off_surface} points")
        assert bad[(1, 0, 0)] >= 1 and bad[(1, 1, 1)] >= 1
        # and through the whole brute force, one vote and three
        for vote3 in (False, True):
            exp = brute_force_signed(p, np.inf, verts, vote3=vote3)
            assert np.array_equal(exp["inside"][keep].astype(bool), inside[keep])
            assert np.array_equal(np.signbit(exp["t"][keep]), inside[keep])
            assert set(exp["votes"][keep].tolist()) == ({0, 3} if vote3 else {0, 1})  # closed: unanimous


def test_icosphere():
    verts = icosphere_verts(2)
    assert verts.shape == (320, 3, 3)
    assert np.linalg.norm(verts.astype(np.float64).mean(axis=1), axis=1).min() > 0.97
    p, inside = shell_points(2000)
    for vote3 in (False, True):
        exp = brute_force_signed(p, np.inf, verts, vote3=vote3)
        assert np.array_equal(exp["inside"].astype(bool), inside), vote3
        assert np.array_equal(np.signbit(exp["t"]), inside)
        # |t| is the distance to the faceted sphere: within its sagitta of | |p| - 1 |
        r = np.linalg.norm(p.astype(np.float64), axis=1)
        assert (np.abs(np.abs(exp["t"]) - np.abs(r - 1.0)) < 0.05).all()


# ---- 2. the rules ------------------------------------------------------------------------------------------
def test_open_mesh_gives_mixed_votes():
    verts = cube_verts(drop_face=1)  # the face x = +1 is missing
    assert verts.shape[0] == 10
    p = grid_points()
    exp = brute_force_signed(p, np.inf, verts, vote3=True)
    mixed = (exp["votes"] == 1) | (exp["votes"] == 2)
    assert mixed.sum() > 100
    assert np.array_equal(exp["inside"], (exp["votes"] >= 2).astype(np.uint8))
    one = brute_force_signed(p, np.inf, verts, vote3=False)
    assert np.array_equal(one["votes"], (exp["counts"][:, 0] & 1).astype(np.uint8)) and one["votes"].max() == 1
    assert (one["counts"][:, 1:] == 0).all()
    derived = one_vote_of(exp)  # the GPU tests' shortcut gives the same answers
    assert all(np.array_equal(derived[k].view(np.uint32) if derived[k].dtype == F else derived[k],
                              one[k].view(np.uint32) if one[k].dtype == F else one[k]) for k in one)


def test_rules():
    verts = cube_verts()
    # beyond rmax on both sides: the miss record, -inf inside and +inf outside
    p = F([[0, 0, 0], [0.25, -0.5, 0.125], [3, 0, 0], [0, -2.5, 1]])
    exp = brute_force_signed(p, 0.25, verts)
    assert exp["t"].tolist() == [-np.inf, -np.inf, np.inf, np.inf]
    assert (exp["tri_id"] == NO_TRI).all() and not exp["u"].any() and not exp["v"].any()
    assert exp["inside"].tolist() == [1, 1, 0, 0]
    # within rmax: the closest-point record, signed
    exp = brute_force_signed(p, np.inf, verts)
    ref = brute_force(p, np.inf, verts)
    assert np.array_equal(np.abs(exp["t"]), ref["t"]) and exp["t"].tolist() == [-1.0, -0.5, 2.0, 1.5]
    assert np.array_equal(exp["tri_id"], ref["tri_id"]) and np.array_equal(exp["u"], ref["u"])
    # on the surface: +0 or -0, whichever the parity says
    s = F([[1, 0.25, 0.5], [-1, 0.25, 0.5], [0.5, 1, -0.25], [0.125, 0.5, -1]])
    exp = brute_force_signed(s, np.inf, verts, vote3=True)
    assert (exp["t"] == 0).all()
    assert np.array_equal(np.signbit(exp["t"]), exp["inside"].astype(bool))
    dd, _, _, _ = tri_nearest(s[:, None, :], verts[None, :, 0], verts[None, :, 1], verts[None, :, 2])
    assert (dd.min(axis=1) == 0).all()
    # invalid points: outside, the +inf miss record, vote 0
    bad = F([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    rmax = F([1, 1, 1, np.nan, 0, -1, 1])
    exp = brute_force_signed(bad, rmax, verts, vote3=True)
    assert exp["inside"].tolist() == [0, 0, 0, 0, 0, 0, 1] and exp["votes"].tolist() == [0, 0, 0, 0, 0, 0, 3]
    assert np.isposinf(exp["t"][:6]).all() and (exp["tri_id"][:6] == NO_TRI).all() and exp["t"][6] == -1.0
    occ = brute_force_signed(bad, rmax, verts, distance=False, vote3=True)  # occupancy does not read rmax
    assert occ["inside"].tolist() == [0, 0, 0, 1, 1, 1, 1] and "t" not in occ
    # the empty scene: every point outside
    exp = brute_force_signed(p, np.inf, np.zeros((0, 3, 3), F), vote3=True)
    assert not exp["inside"].any() and not exp["votes"].any() and np.isposinf(exp["t"]).all()
    # a closed mesh added twice: parity flips back
    exp = brute_force_signed(p, np.inf, np.concatenate([verts, verts]), vote3=True)
    assert not exp["inside"].any() and (exp["counts"][:2] == 2).all()


# ---- 3. the ABI --------------------------------------------------------------------------------------------
def test_constants_and_prototypes():
    assert (_lib.SIGNED_DISTANCE, _lib.SIGNED_OCCUPANCY, _lib.SIGNED_VOTE3) == (0, 1, 1)
    header = open(_lib.HEADER).read()
    for line in ("#define BM_SIGNED_DISTANCE 0u", "#define BM_SIGNED_OCCUPANCY 1u", "#define BM_SIGNED_VOTE3 1u"):
        assert line in header
    assert C.sizeof(_lib.Point) == 16 and _lib.Point.rmax.offset == 12
    P, U = C.c_void_p, C.c_uint32
    assert _lib.SIGNATURES["bm_scene_signed_distances"] == (C.c_int32, [P, P, U, U, U, P, P])
    assert _lib.SIGNATURES["bm_scene_signed_distances_counters"] == (C.c_int32,
                                                                    [P, P, U, U, U, P, P, C.POINTER(C.c_uint64)])
    assert {"bm_scene_signed_distances", "bm_scene_signed_distances_counters"} <= set(_lib.declared_symbols())
    lib = _lib.load()
    assert lib.bm_scene_signed_distances and lib.bm_scene_signed_distances_counters  # exported by the .so


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 4)()
    bad = _lib.ERROR_INVALID_PARAMETER
    for mode in (_lib.SIGNED_DISTANCE, _lib.SIGNED_OCCUPANCY, 2):
        for flags in (0, _lib.SIGNED_VOTE3, 2):
            assert lib.bm_scene_signed_distances(None, None, 0, mode, flags, None, None) == bad
            assert lib.bm_scene_signed_distances(None, None, 16, mode, flags, None, None) == bad
            assert lib.bm_scene_signed_distances_counters(None, None, 0, mode, flags, None, None, out) == bad
            assert lib.bm_scene_signed_distances_counters(None, None, 0, mode, flags, None, None, None) == bad


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::signedDistances of include/beam/Beam.h compiles and links against the library."""
    src = tmp_path / "signed.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "signed"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()
