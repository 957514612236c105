"""Ray queries (bm_scene_trace_rays): the ABI's record layouts, null handling and the C++ layer (CPU)."""
import ctypes as C
import os
import subprocess

from raytracercuda_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <beam/Beam.h>
static_assert(sizeof(bm_ray) == 32 && sizeof(bm_hit) == 16, "record sizes");
int main() {
    auto scene = Beam::IScene::create();  // no device here: null
    if (!scene) return 0;
    const Beam::u32 a = scene->traceRays(nullptr, 0, nullptr);
    const Beam::u32 b = scene->occluded(nullptr, 0, nullptr, 0);
    return (int)(a + b);
}
"""


def test_record_sizes():
    assert C.sizeof(_lib.Ray) == 32 and C.sizeof(_lib.Hit) == 16
    assert _lib.Ray.tmax.offset == 12 and _lib.Ray.dir.offset == 16 and _lib.Hit.tri_id.offset == 12


def test_null_scene_without_a_device():
    lib = _lib.load()
    out = (C.c_uint64 * 3)()
    for mode in (_lib.RAYS_CLOSEST, _lib.RAYS_ANY_HIT):
        assert lib.bm_scene_trace_rays(None, None, 0, mode, 0, None) == _lib.ERROR_INVALID_PARAMETER
        assert lib.bm_scene_trace_rays(None, None, 16, mode, 0, None) == _lib.ERROR_INVALID_PARAMETER
        assert lib.bm_scene_trace_rays_counters(None, None, 0, mode, 0, None, out) == _lib.ERROR_INVALID_PARAMETER
    assert lib.bm_scene_trace_rays_counters(None, None, 0, 0, 0, None, None) == _lib.ERROR_INVALID_PARAMETER


def test_cpp_layer_compiles_and_links(tmp_path):
    """IScene::traceRays and IScene::occluded of include/beam/Beam.h compile and link against the library."""
    src = tmp_path / "rays.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "rays"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    assert exe.exists()
