"""Hit attributes (bm_scene_hit_attributes): the request record's layout, the constants, null handling and
the C++ layer (CPU)."""
import ctypes as C
import os
import re
import subprocess

from raytracercuda_amd import _lib, beam

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SNIPPET = r"""
#include <cstddef>
#include <cstdio>
#include <beam/Beam.h>
static_assert(sizeof(bm_attr_req) == 24, "record size");
Beam::u32 shading_normals(Beam::IScene& scene, const bm_hit* hits, Beam::u32 n, float* out) {  // compiled, not run
    bm_attr_req r = {BM_VERTEX_DATA_NORMAL, 3, BM_ATTR_NORMALIZE, 0, out};
    return scene.hitAttributes(hits, n, &r, 1);
}
int main(int argc, char**) {
    std::printf("%zu %zu %zu %zu %zu %zu\n", sizeof(bm_attr_req), offsetof(bm_attr_req, slot),
                offsetof(bm_attr_req, components), offsetof(bm_attr_req, flags), offsetof(bm_attr_req, pad),
                offsetof(bm_attr_req, out_dev));
    if (argc > 1000) {  // never: the call only has to compile and link here (no device is touched)
        auto scene = Beam::IScene::create();
        return (int)shading_normals(*scene, nullptr, 0, nullptr);
    }
    // the C entry point itself rejects a null scene before it looks at anything else
    bm_attr_req r = {BM_VERTEX_DATA_NORMAL, 3, 0, 0, nullptr};
    return bm_scene_hit_attributes(nullptr, nullptr, 0, &r, 1) == BM_ERROR_INVALID_PARAMETER ? 0 : 1;
}
"""


def header_constants():
    text = open(_lib.HEADER).read()
    return {k: int(v, 0) for k, v in re.findall(r"^#define (BM_(?:ATTR|VERTEX_DATA)_\w+) (\w+?)u?\b", text, re.M)}


def test_request_record_matches_the_header(tmp_path):
    """sizeof(bm_attr_req) == 24 and every field of _lib.AttrReq sits where the C compiler puts it."""
    assert C.sizeof(_lib.AttrReq) == 24
    src = tmp_path / "attrs.cpp"
    src.write_text(SNIPPET)
    exe = tmp_path / "attrs"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                    _lib.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(_lib.LIB_PATH)}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    size, *offsets = map(int, out.stdout.split())
    r = _lib.AttrReq
    assert size == C.sizeof(r)
    assert offsets == [r.slot.offset, r.components.offset, r.flags.offset, r.pad.offset, r.out_dev.offset]
    assert offsets == [0, 4, 8, 12, 16]


def test_constants_equal_the_header():
    h = header_constants()
    assert h["BM_ATTR_GEOM_NORMAL"] == beam.ATTR_GEOM_NORMAL == 16
    assert h["BM_ATTR_MESH_FACE"] == beam.ATTR_MESH_FACE == 17
    assert h["BM_ATTR_NORMALIZE"] == beam.ATTR_NORMALIZE == 1
    assert h["BM_ATTR_MAX_REQS"] == beam.ATTR_MAX_REQS == 4
    for name in ("POSITION", "NORMAL", "UV1", "UV2", "TANGENT", "BITANGENT", "EXTRA1", "EXTRA2", "EXTRA3", "EXTRA4",
                 "COUNT"):
        assert h["BM_VERTEX_DATA_" + name] == getattr(beam, "VERTEX_DATA_" + name), name
    # the pseudo-slots lie outside the vertex slots
    assert beam.ATTR_GEOM_NORMAL >= beam.VERTEX_DATA_COUNT and beam.ATTR_MESH_FACE >= beam.VERTEX_DATA_COUNT


def test_symbol_resolves_and_is_declared():
    lib = _lib.load()
    assert "bm_scene_hit_attributes" in _lib.declared_symbols()
    assert "bm_scene_hit_attributes" in _lib.SIGNATURES
    assert lib.bm_scene_hit_attributes is not None


def test_null_scene_without_a_device():
    lib = _lib.load()
    req = (_lib.AttrReq * 1)()
    req[0].slot, req[0].components = _lib.VERTEX_DATA_NORMAL, 3
    bad = _lib.ERROR_INVALID_PARAMETER
    assert lib.bm_scene_hit_attributes(None, None, 0, req, 1) == bad
    assert lib.bm_scene_hit_attributes(None, None, 16, req, 1) == bad
    assert lib.bm_scene_hit_attributes(None, None, 0, None, 0) == bad
