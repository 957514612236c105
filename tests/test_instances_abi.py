"""Instance transforms (bm_scene_add_instance and its companions): the symbols, null handling, the C++ layer,
bm_xform_normal_matrix against a numpy restatement, and beam.py's transform shapes (CPU).

The restatement is the header's arithmetic in numpy float32, one operation per statement so that nothing fuses:
position rows ((x0*px + x1*py) + x2*pz) + x3, normal rows (c0*nx + c1*ny) + c2*nz with c the cofactor matrix of
the linear part. tests/test_gpu_instances.py pre-transforms its meshes with it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from raytracercuda_amd import _lib, beam

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAD = _lib.ERROR_INVALID_PARAMETER
SYMBOLS = ("bm_scene_add_instance", "bm_scene_set_instance_transform", "bm_scene_get_instance_transform",
           "bm_scene_remove_instance", "bm_xform_normal_matrix", "bm_model_add_instance")


# ---- the restatement ---------------------------------------------------------------------------------
def normal_matrix_np(x):
    """The cofactor matrix of the transform's linear part, (3,3) float32: each entry a*b - c*d as two
    products and one difference."""
    x = np.asarray(x, F).reshape(3, 4)
    L = x[:, :3]

    def cof(a, b, c, d):
        p = F(L[a] * L[b])
        q = F(L[c] * L[d])
        return F(p - q)

    return np.array([[cof((1, 1), (2, 2), (1, 2), (2, 1)), cof((1, 2), (2, 0), (1, 0), (2, 2)),
                      cof((1, 0), (2, 1), (1, 1), (2, 0))],
                     [cof((0, 2), (2, 1), (0, 1), (2, 2)), cof((0, 0), (2, 2), (0, 2), (2, 0)),
                      cof((0, 1), (2, 0), (0, 0), (2, 1))],
                     [cof((0, 1), (1, 2), (0, 2), (1, 1)), cof((0, 2), (1, 0), (0, 0), (1, 2)),
                      cof((0, 0), (1, 1), (0, 1), (1, 0))]], F)


def xform_positions(x, pos):
    x = np.asarray(x, F).reshape(3, 4)
    p = np.ascontiguousarray(pos, F).reshape(-1, 3)
    out = np.empty_like(p)
    for r in range(3):
        a = x[r, 0] * p[:, 0]
        b = x[r, 1] * p[:, 1]
        s = a + b
        c = x[r, 2] * p[:, 2]
        s = s + c
        out[:, r] = s + x[r, 3]
    assert out.dtype == F
    return out


def xform_normals(x, nrm):
    c9 = normal_matrix_np(x)
    n = np.ascontiguousarray(nrm, F).reshape(-1, 3)
    out = np.empty_like(n)
    for r in range(3):
        a = c9[r, 0] * n[:, 0]
        b = c9[r, 1] * n[:, 1]
        s = a + b
        c = c9[r, 2] * n[:, 2]
        out[:, r] = s + c
    assert out.dtype == F
    return out


def xform_mesh(x, m):
    """The mesh dict with positions and normals through the transform; everything else as it is."""
    return dict(m, pos=xform_positions(x, m["pos"]), nrm=xform_normals(x, m["nrm"]))


def rotation(axis, angle, t=(0, 0, 0)):
    """A (3,4) float32 rotation about axis by angle (Rodrigues, in float64, rounded once) plus translation."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return np.concatenate([r, np.asarray(t, np.float64).reshape(3, 1)], axis=1).astype(F)


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(F)
ROTATION = rotation((1, 2, 3), 0.7, (0.5, -0.25, 2.0))
SCALE = np.array([[2.5, 0, 0, 0.1], [0, 0.5, 0, -0.2], [0, 0, 1.25, 0.3]], F)
MIRROR = np.array([[-1, 0, 0, 0.75], [0, 1, 0, 0], [0, 0, 1, 0]], F)
SINGULAR = np.array([[1, 2, 3, 0], [2, 4, 6, 1], [0.5, -1, 0.25, 2]], F)  # row 1 = 2 * row 0


def lib_normal_matrix(x):
    lib = _lib.load()
    x = np.ascontiguousarray(x, F).reshape(12)
    out = np.full(9, np.nan, F)
    fp = C.POINTER(C.c_float)
    assert lib.bm_xform_normal_matrix(x.ctypes.data_as(fp), out.ctypes.data_as(fp)) == 0
    return out.reshape(3, 3)


# ---- symbols and null handling -----------------------------------------------------------------------
def test_symbols_are_declared_bound_and_resolve():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def test_null_handles_and_matrices_without_a_device():
    lib = _lib.load()
    fp = C.POINTER(C.c_float)
    x = np.ascontiguousarray(IDENTITY).reshape(12)
    xp = x.ctypes.data_as(fp)
    out = np.zeros(12, F)
    idx = C.c_uint32(7)
    assert lib.bm_scene_add_instance(None, None, xp, C.byref(idx)) == BAD
    assert lib.bm_scene_add_instance(None, None, None, None) == BAD
    assert idx.value == 7
    assert lib.bm_scene_set_instance_transform(None, 0, xp) == BAD
    assert lib.bm_scene_set_instance_transform(None, 0, None) == BAD
    assert lib.bm_scene_get_instance_transform(None, 0, out.ctypes.data_as(fp)) == BAD
    assert lib.bm_scene_remove_instance(None, 0) == BAD
    assert lib.bm_xform_normal_matrix(None, out.ctypes.data_as(fp)) == BAD
    assert lib.bm_xform_normal_matrix(xp, None) == BAD
    assert lib.bm_model_add_instance(None, None, None, xp) == BAD
    assert lib.bm_model_add_instance(None, None, None, None) == BAD


# ---- the C++ layer -----------------------------------------------------------------------------------
SNIPPET = r"""
#include <cstdio>
#include <beam/Beam.h>
Beam::u32 place(Beam::IScene& scene, Beam::IMesh* mesh, const float* colMajor16) {  // compiled, not run
    float x[12], back[12];
    Beam::xformFromColumnMajor4x4(colMajor16, x);
    Beam::u32 index = 0;
    Beam::u32 e = scene.addInstance(mesh, x, &index);
    if (e == Beam::ERROR_ALL_FINE) e = scene.setInstanceTransform(index, x);
    if (e == Beam::ERROR_ALL_FINE) e = scene.instanceTransform(index, back);
    if (e == Beam::ERROR_ALL_FINE) e = scene.removeInstance(index);
    return e;
}
int main(int argc, char**) {
    // glm::mat4's memory: columns (1,2,3,0) (4,5,6,0) (7,8,9,0) and the translation (10,11,12,1)
    const float m[16] = {1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0, 10, 11, 12, 1};
    float x[12], c[9];
    Beam::xformFromColumnMajor4x4(m, x);
    for (int i = 0; i < 12; ++i) std::printf("%g ", x[i]);
    if (Beam::normalMatrix(x, c) != Beam::ERROR_ALL_FINE) return 2;
    std::printf("\n");
    if (argc > 1000) {  // never: the calls only have to compile and link here (no device is touched)
        auto scene = Beam::IScene::create();
        auto mesh = Beam::IMesh::create();
        scene->addInstance(mesh, x);
        return (int)place(*scene, mesh.get(), m);
    }
    return bm_scene_add_instance(nullptr, nullptr, x, nullptr) == BM_ERROR_INVALID_PARAMETER ? 0 : 1;
}
"""


def test_cpp_layer_compiles_links_and_converts_column_major(tmp_path):
    src = tmp_path / "inst.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "inst"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [float(v) for v in out.stdout.split()] == [1, 4, 7, 10, 2, 5, 8, 11, 3, 6, 9, 12]


# ---- bm_xform_normal_matrix --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["IDENTITY", "ROTATION", "SCALE", "MIRROR", "SINGULAR"])
def test_normal_matrix_is_bit_equal_to_the_restatement(name):
    x = globals()[name]
    got, exp = lib_normal_matrix(x), normal_matrix_np(x)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (name, got, exp)
    assert np.array_equal(beam.normal_matrix(x).view(np.uint32), exp.view(np.uint32))


def test_normal_matrix_random_matrices_bit_equal():
    rng = np.random.default_rng(2025)
    xs = rng.normal(size=(1000, 3, 4)).astype(F)
    xs[::7] *= F(1e-3)
    xs[3::11] *= F(1e4)
    for x in xs:
        got, exp = lib_normal_matrix(x), normal_matrix_np(x)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), x


def test_normal_matrix_special_cases():
    assert np.array_equal(lib_normal_matrix(IDENTITY), np.eye(3, dtype=F))
    # a rotation's cofactor matrix is the rotation itself (det 1, inverse = transpose), within float rounding:
    # every entry is two products of entries bounded by 1 and one difference, each within half an ulp of 1
    c = lib_normal_matrix(ROTATION)
    assert np.max(np.abs(c.astype(np.float64) - ROTATION[:, :3].astype(np.float64))) <= 4 * np.finfo(F).eps
    # scale: diag(sy*sz, sx*sz, sx*sy); mirror: det < 0 flips the normals' sign convention (not fixed up)
    assert np.array_equal(lib_normal_matrix(SCALE), np.diag(F([0.5 * 1.25, 2.5 * 1.25, 2.5 * 0.5])).astype(F))
    assert np.array_equal(lib_normal_matrix(MIRROR), np.diag(F([1, -1, -1])))
    # singular: C . L^T = det * I = 0 within rounding, and C itself is finite
    cs = lib_normal_matrix(SINGULAR).astype(np.float64)
    assert np.isfinite(cs).all() and np.max(np.abs(cs @ SINGULAR[:, :3].astype(np.float64).T)) < 1e-4


# ---- beam.py's transform shapes ----------------------------------------------------------------------
def test_accepted_and_rejected_xform_shapes():
    flat = ROTATION.reshape(12)
    four = np.concatenate([ROTATION, F([[0, 0, 0, 1]])])
    for ok in (flat, list(map(float, flat)), tuple(flat), ROTATION, ROTATION.tolist(), four, four.astype(np.float64)):
        x = beam._xform12(ok)
        assert x.dtype == F and x.shape == (12,) and x.flags["C_CONTIGUOUS"]
        assert np.array_equal(x, flat)
        assert beam.normal_matrix(ok).shape == (3, 3)
    assert np.array_equal(beam._xform12(np.asfortranarray(ROTATION)), flat)  # by value, not by memory order
    bad_row = four.copy()
    bad_row[3, 3] = F(1.0000001)
    proj = four.copy()
    proj[3, 0] = F(0.5)
    for bad in (flat[:11], np.zeros(16, F), np.zeros((4, 3), F), np.zeros((3, 3), F), np.zeros((2, 6), F),
                np.zeros((1, 12), F), bad_row, proj, F(1.0), [], None):
        with pytest.raises(ValueError):
            beam._xform12(bad)
        with pytest.raises(ValueError):
            beam.normal_matrix(bad)
