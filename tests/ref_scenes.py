"""Small designed scenes for the per-pixel pins against the reference's own CPU path (tests/golden/ref).

Shared by tests/golden/make_ref_frames.py, which traces them with the reference's binary, and by the
tests, which check that the meshes stored in the fixtures are the ones built here. Everything is
float32, finite, with non-zero normals, from seeded numpy.

A scene is {"meshes": [{"pos", "nrm", "idx"}, ...], "w", "h", "cam": (left, right, top, bottom, zoom),
"views": [(eye, orient9 column-major), ...]}.

The reference's tree: leaves are the cells of a grid over [-30, 30]^3, 60/2048 wide in x
and 60/1024 in y and z; a leaf keeps the first 256 faces inserted.
"""
import numpy as np

CELL_X = 60.0 / 2048.0
CELL_YZ = 60.0 / 1024.0

IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
# the matrices of test_gpu_reference_mode.py (column-major): dir = (rz, ry, 0) and dir = (rx, rz, rz)
FLAT_X = (0, 0, 0, 0, 1, 0, 1, 0, 0)
FLAT_Y = (1, 0, 0, 0, 0, 0, 0, 1, 1)
# a zero row proper: dir.x == 0, dir.y == 0 for every ray
ZERO_X = (0, 0, 0, 0, 1, 0, 0, 0, 1)
ZERO_Y = (1, 0, 0, 0, 0, 0, 0, 0, 1)
ROLL_90 = (0, 1, 0, -1, 0, 0, 0, 0, 1)  # dir = (-ry, rx, rz)
SHEAR = (1.0, 0.2, 0.1, 0.3, 1.1, -0.2, 0.0, 0.0, 0.9)  # neither orthogonal nor unit columns
SQUARE = (-1.0, 1.0, -1.0, 1.0, 1.0)


def _rot_y(deg):
    a = np.deg2rad(deg)
    c, s = float(np.cos(a)), float(np.sin(a))
    return (c, 0, -s, 0, 1, 0, s, 0, c)  # columns (c,0,-s), (0,1,0), (s,0,c): +z turns towards +x


def soup(tris, nrms):
    """Unshared mesh of triangles tris[n,3,3] with per-corner normals nrms[n,3,3] (or per-face [n,3])."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    nrms = np.asarray(nrms, np.float32)
    if nrms.ndim == 2:
        nrms = np.repeat(nrms[:, None, :], 3, axis=1)
    n = tris.shape[0]
    return {"pos": tris.reshape(-1, 3).copy(), "nrm": nrms.reshape(-1, 3).astype(np.float32),
            "idx": np.arange(3 * n, dtype=np.uint32)}


def blob(seed, n_lat, n_lon, center, radius, bump=0.15):
    """A bumpy sphere open at the poles with shared vertices: 2 * n_lat * n_lon triangles."""
    rng = np.random.default_rng(seed)
    lat = np.linspace(0.06 * np.pi, 0.94 * np.pi, n_lat + 1)
    lon = np.arange(n_lon) * (2.0 * np.pi / n_lon)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    unit = np.stack([np.sin(la) * np.cos(lo), np.cos(la), np.sin(la) * np.sin(lo)], -1).reshape(-1, 3)
    r = radius * (1.0 + bump * rng.uniform(-1.0, 1.0, size=(unit.shape[0], 1)))
    pos = (np.asarray(center, np.float64) + unit * r).astype(np.float32)
    nrm = (unit + 0.3 * rng.uniform(-1.0, 1.0, size=unit.shape)).astype(np.float32)
    idx = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            c, d = a + n_lon, b + n_lon
            idx += [a, c, b, b, c, d]
    return {"pos": pos, "nrm": nrm, "idx": np.asarray(idx, np.uint32)}


def _cap():
    """300 and 600 small triangles, each group strictly inside one leaf cell, stacked along the view axis
    with the nearest ones inserted last: the 44 and 344 faces the 256-face cap drops are exactly the ones
    a closest hit returns."""
    rng = np.random.default_rng(101)
    tris, nrms = [], []
    for cell_x, count in ((10, 300), (12, 600)):
        cx = (cell_x + 0.5) * CELL_X
        cy = 3.5 * CELL_YZ
        z_far, z_near = 3.9 * CELL_YZ, 3.1 * CELL_YZ  # inside z cell 3: [3, 4) * CELL_YZ
        for i in range(count):
            z = z_far + (z_near - z_far) * i / (count - 1)
            j = rng.uniform(-0.002, 0.002, size=(3, 2))
            tris.append([[cx - 0.008 + j[0, 0], cy - 0.008 + j[0, 1], z],
                         [cx + 0.008 + j[1, 0], cy - 0.008 + j[1, 1], z],
                         [cx + j[2, 0], cy + 0.010 + j[2, 1], z]])
            n = rng.uniform(-1.0, 1.0, size=3)
            n[2] = rng.uniform(0.05, 1.0) * (1 if i % 2 else -1)
            nrms.append(n)
    mid = 11.5 * CELL_X
    views = [((mid, 3.5 * CELL_YZ, -1.0), IDENTITY),
             ((mid - 0.02, 3.5 * CELL_YZ + 0.01, -0.8), IDENTITY),
             ((mid + 0.3, 3.5 * CELL_YZ, -0.9), _rot_y(-16.0))]
    return {"meshes": [soup(tris, nrms)], "w": 96, "h": 48, "cam": (-0.06, 0.06, -0.03, 0.03, 1.0), "views": views}


def _ties():
    """Exact-t ties: coincident duplicates with different normals in one mesh (ids 0, 1) and across two
    meshes (ids 3, 7), the same triangle with its corners rotated (id 8), two coplanar triangles sharing
    a diagonal (0, 2), a roof whose ridge lies in the plane x = 0 (4, 5) and a triangle in that plane
    (6): with dir.x == 0 from an eye at x = 0 every ray runs inside that plane, hits the ridge on the
    shared edge of both roof triangles, and meets triangle 6 edge-on (det == 0: 1/det is infinite)."""
    t0 = [[-1, -1, 2], [1, -1, 2], [-1, 1, 2]]
    t3 = [[1.5, -1, 2.5], [3, -1, 2.5], [1.5, 1, 2.5]]
    m0 = soup([t0, t0, [[1, -1, 2], [1, 1, 2], [-1, 1, 2]], t3,
               [[0, -0.5, 1.5], [0, 0.5, 1.5], [-0.5, 0, 1.8]],
               [[0, 0.5, 1.5], [0, -0.5, 1.5], [0.5, 0, 1.8]],
               [[0, 0.6, 1.0], [0, 0.9, 1.0], [0, 0.75, 1.3]]],
              [[0, 0, 1], [1, 0, 1], [0, 1, 1], [0, 0, 1], [1, 0, 2], [-1, 0, 3], [1, 1, 1]])
    m1 = soup([t3, [[1, -1, 2], [-1, 1, 2], [-1, -1, 2]]], [[1, 0, 0.25], [0.5, 0.5, 0.5]])
    views = [((0.0, 0.0, -1.0), IDENTITY), ((0.0, 0.0, -1.0), ZERO_X), ((0.5, 0.2, -1.5), _rot_y(12.0)),
             ((2.25, 0.0, -1.0), IDENTITY)]
    return {"meshes": [m0, m1], "w": 64, "h": 48, "cam": SQUARE, "views": views}


def _early_out():
    """One large slanted triangle over hundreds of leaves with small triangles just in front of and
    behind it: a ray that crosses a leaf holding the large triangle takes its hit there, wherever on
    the triangle that hit lies, and never reaches the leaf of a nearer small triangle."""
    rng = np.random.default_rng(202)
    big = np.array([[-0.4, -0.3, 1.0], [0.4, -0.3, 1.6], [0.0, 0.4, 1.3]])
    n = np.cross(big[1] - big[0], big[2] - big[0])
    n /= np.linalg.norm(n)
    tris, nrms = [big], [[0.2, 0.1, 1.0]]
    for i in range(500):
        w = rng.dirichlet((1.0, 1.0, 1.0))
        c = w @ big + n * rng.uniform(0.004, 0.05) * (1 if i % 3 else -1)
        tris.append(c + rng.uniform(-0.02, 0.02, size=(3, 3)))
        nrms.append(rng.uniform(-1.0, 1.0, size=3) + [0, 0, 1.5])
    views = [((0.0, 0.0, -0.5), IDENTITY), ((1.4, 0.1, 0.2), _rot_y(-50.0)), ((-1.2, 0.5, 0.0), _rot_y(42.0)),
             ((0.9, -0.4, 2.6), _rot_y(-140.0))]
    return {"meshes": [soup(tris, nrms)], "w": 128, "h": 96, "cam": (-0.5, 0.5, -0.4, 0.4, 1.0), "views": views}


def _axis_rays():
    """Rays with zero direction components and eyes on split planes (x = 0, x = 15, y = 7.5) or exactly
    on a leaf corner: the slab test divides by zero there and the near/far child choice sits on `p < s`."""
    meshes = [blob(301, 12, 24, (0, 0, 0), 1.0), blob(302, 8, 16, (15, 0, 0), 0.7), blob(303, 8, 16, (0, 7.5, 0), 0.7)]
    corner = (10 * CELL_X, 3 * CELL_YZ, -30.0 + 461 * CELL_YZ)
    views = [((-3.0, 0.0, 0.0), FLAT_X), ((0.0, -3.0, -3.0), FLAT_Y), ((15.0, -3.0, -3.0), FLAT_Y),
             ((-3.0, 7.5, 0.0), FLAT_X), ((15.0, 0.0, -3.0), FLAT_X), ((0.0, 7.5, 0.0), FLAT_Y),
             ((0.0, 0.0, -3.0), ZERO_X), ((0.0, 0.0, -3.0), ZERO_Y), ((15.0, 0.0, -3.0), ZERO_X),
             ((0.0, 7.5, -3.0), ZERO_Y), ((15.0, 0.0, -3.0), IDENTITY), ((0.0, 7.5, -3.0), IDENTITY),
             ((0.0, 0.0, -3.0), ROLL_90), (corner, IDENTITY)]
    return {"meshes": meshes, "w": 64, "h": 48, "cam": SQUARE, "views": views}


def _world_box():
    """The +-30 world box: eyes outside it, slivers that cross its faces with coordinates of a few
    hundred, a mesh between an outside eye and the box and one beyond the far face (neither enters the
    reference's tree)."""
    sl = soup([[[29.0, -0.5, 0.0], [300.0, 0.0, 0.3], [29.0, 0.5, 0.0]],
               [[-0.6, -0.5, 29.0], [0.6, -0.5, 29.0], [0.1, 0.2, 250.0]],
               [[-2.5, 2.0, -29.0], [-2.0, 2.0, -29.0], [-2.2, 2.4, -400.0]]],
              [[0.3, 0.1, 1.0], [0.0, 1.0, 0.4], [1.0, 0.0, 0.6]])
    meshes = [blob(401, 10, 20, (0, 0, 0), 2.0), sl, blob(402, 6, 12, (1.5, 0.5, -34.0), 0.4),
              blob(403, 6, 12, (-1.0, -1.0, 45.0), 1.0)]
    views = [((0.0, 0.0, -40.0), IDENTITY), ((0.0, 0.0, -29.0), IDENTITY), ((29.5, 0.0, -20.0), IDENTITY),
             ((-35.0, 0.0, -35.0), _rot_y(45.0)), ((0.0, 0.0, 20.0), IDENTITY), ((-2.2, 2.2, -60.0), IDENTITY)]
    return {"meshes": meshes, "w": 80, "h": 64, "cam": (-0.08, 0.08, -0.064, 0.064, 1.0), "views": views}


def _camera(which):
    """setInitialRays with an off-centre frustum, zoom 0.5 / 2.5 and frame sizes that are no multiple of
    8: the ray table is a sequential `+=` recurrence (Camera.cpp:51-66), so its rounding depends on all
    of them; and a sheared orient."""
    meshes = [blob(501, 14, 28, (0.1, -0.1, 0.0), 1.0)]
    if which == "a":
        w, h, cam = 101, 37, (-0.7, 1.1, 0.9, -0.4, 0.5)
        views = [((0.0, 0.0, -1.6), IDENTITY), ((0.3, -0.2, -1.5), SHEAR)]
    else:
        w, h, cam = 75, 50, (-1.3, 0.4, -0.2, 0.8, 2.5)
        views = [((1.2, -0.5, -6.0), IDENTITY), ((0.9, -0.4, -5.0), SHEAR)]
    return {"meshes": meshes, "w": w, "h": h, "cam": cam, "views": views}


def _meshes():
    """Three meshes of unequal size, shared and unshared vertices, global id order unlike the spatial
    order: the nearest mesh comes last, the unshared one in the middle."""
    rng = np.random.default_rng(601)
    c = rng.uniform(-0.5, 0.5, size=(50, 1, 3)) + [-1.2, 0.0, 0.3]
    loose = soup(c + rng.uniform(-0.15, 0.15, size=(50, 3, 3)), rng.uniform(-1.0, 1.0, size=(50, 3, 3)) + [0, 0, 1.2])
    meshes = [blob(602, 12, 25, (1.2, 0.0, 0.5), 0.8), loose, blob(603, 5, 25, (0.2, 0.1, -0.8), 0.5)]
    views = [((0.0, 0.0, -4.0), IDENTITY), ((4.0, 0.5, -1.0), _rot_y(-75.0)), ((-3.0, -0.2, -2.5), _rot_y(48.0))]
    return {"meshes": meshes, "w": 96, "h": 64, "cam": (-0.75, 0.75, -0.5, 0.5, 1.0), "views": views}


BUILDERS = {
    "cap": _cap, "ties": _ties, "early_out": _early_out, "axis_rays": _axis_rays, "world_box": _world_box,
    "camera_a": lambda: _camera("a"), "camera_b": lambda: _camera("b"), "meshes": _meshes,
}
DESIGNED = tuple(BUILDERS)


def build(name):
    s = BUILDERS[name]()
    s["views"] = [(tuple(np.float32(e).tolist()), tuple(np.float32(o).tolist())) for e, o in s["views"]]
    for m in s["meshes"]:
        assert np.isfinite(m["pos"]).all() and np.isfinite(m["nrm"]).all()
        assert (np.abs(m["nrm"]).max(axis=1) > 0).all()
    return s
