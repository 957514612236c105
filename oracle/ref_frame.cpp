// ref_frame.cpp — TEST INFRASTRUCTURE ONLY (oracle/, never linked into the product).
//
// Driver for the reference's own CPU-emulation path (`#define CUDA 0`), which oracle/Makefile's target
// ref_frame compiles from the reference's sources beside this file. It reads a
// scene, drives the reference through its public API (Beam.h) only, and writes the framebuffers the
// reference computes, so that tests/golden/make_ref_frames.py can record them pixel by pixel.
//
//   ref_frame SCENE.bin FRAMES.bin      (stdout: the reference's own build report, pass by pass)
//
// SCENE.bin (little-endian): "BMREFSC1"; u32 num_meshes; per mesh u32 num_verts, u32 num_idx,
//   f32 pos[3*num_verts], f32 nrm[3*num_verts], u32 idx[num_idx]; u32 width, height;
//   f32 left, right, top, bottom, zoom (Camera::setInitialRays); u32 num_views; per view f32 eye[3],
//   f32 orient[9] (column-major mat3, as traceScene takes it).
// FRAMES.bin: u32 num_passes, num_views, width, height; then u32 frame[width*height] per pass and view.
//
// Pass 0 traces the meshes as given (the real normals). The reference has no output for the triangle
// it hit, so passes 1..P (P = ceil(log2 N_tri), at least 1) read the id bit by bit (Appendix A.3):
// pass b+1 gives every face three vertices of its own, positions and face order unchanged, with the
// normal (0,0,1) where bit b of the face's global id is set and (1,0,0) elsewhere. The red channel of
// a hit is then 255 or 0. The tree depends on positions and face order alone, so it is the same in
// every pass; the scene is nevertheless created and built anew for each.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Beam.h"
#include "RenderTarget.h"

// ---- the host side of the reference's render target (its RenderTarget.cpp maps an OpenGL buffer) ----

bool bmGLHasContext() { return false; }

static std::vector<Beam::u32> g_pixels;  // what lock() hands out

namespace Beam {
IRenderTarget* RenderTarget::m_RT = nullptr;

RenderTarget::RenderTarget(u32 width, u32 height, u32 pitch)
    : m_cudaGraphicsRT(nullptr), m_pitch(pitch), m_width(width), m_height(height), m_buffer(nullptr) {}

RenderTarget::~RenderTarget() {
    if (m_RT == this) m_RT = nullptr;
}

u32 RenderTarget::lock() {
    if (m_buffer) return ERROR_UNLOCK_FIRST;
    g_pixels.assign((size_t)m_width * m_height, 0xDEADBEEFu);  // a value the trace never writes
    m_buffer = g_pixels.data();
    m_RT = this;
    return ERROR_ALL_FINE;
}

u32 RenderTarget::unlock() {
    if (!m_buffer) return ERROR_LOCK_FIRST;
    m_buffer = nullptr;
    m_RT = nullptr;
    return ERROR_ALL_FINE;
}

IRenderTarget* RenderTarget::get() { return m_RT; }
}  // namespace Beam

// ---- scene file ----

namespace {

struct MeshIn {
    std::vector<float> pos, nrm;
    std::vector<uint32_t> idx;
};
struct View {
    float eye[3], orient[9];
};

void die(const char* what) {
    std::fprintf(stderr, "ref_frame: %s\n", what);
    std::exit(2);
}

template <class T>
void rd(std::FILE* f, T* p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) die("scene file truncated");
}

void must(Beam::u32 err, const char* call) {
    if (err != Beam::ERROR_ALL_FINE) {
        std::fprintf(stderr, "ref_frame: %s returned %u\n", call, err);
        std::exit(3);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: ref_frame SCENE.bin FRAMES.bin");
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) die("cannot open the scene file");
    char magic[8];
    rd(f, magic, 8);
    if (std::memcmp(magic, "BMREFSC1", 8) != 0) die("not a scene file");
    uint32_t num_meshes = 0;
    rd(f, &num_meshes, 1);
    std::vector<MeshIn> meshes(num_meshes);
    uint64_t num_tris = 0;
    for (MeshIn& m : meshes) {
        uint32_t nv = 0, ni = 0;
        rd(f, &nv, 1);
        rd(f, &ni, 1);
        if (ni % 3) die("index count is no multiple of 3");
        m.pos.resize((size_t)nv * 3);
        m.nrm.resize((size_t)nv * 3);
        m.idx.resize(ni);
        rd(f, m.pos.data(), m.pos.size());
        rd(f, m.nrm.data(), m.nrm.size());
        rd(f, m.idx.data(), m.idx.size());
        for (uint32_t i : m.idx)
            if (i >= nv) die("vertex index out of range");
        num_tris += ni / 3;
    }
    uint32_t wh[2];
    float cam[5];
    uint32_t num_views = 0;
    rd(f, wh, 2);
    rd(f, cam, 5);
    rd(f, &num_views, 1);
    std::vector<View> views(num_views);
    for (View& v : views) {
        rd(f, v.eye, 3);
        rd(f, v.orient, 9);
    }
    std::fclose(f);
    const uint32_t w = wh[0], h = wh[1];

    uint32_t planes = 1;
    while ((1ull << planes) < num_tris) ++planes;
    const uint32_t passes = 1 + planes;

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) die("cannot open the output file");
    const uint32_t head[4] = {passes, num_views, w, h};
    std::fwrite(head, 4, 4, out);

    for (uint32_t pass = 0; pass < passes; ++pass) {
        std::printf("== ref_frame pass %u of %u\n", pass, passes);
        std::fflush(stdout);
        // the meshes of this pass: as given, or unshared with the id's bit written into the normals
        std::vector<MeshIn> pm;
        if (pass == 0) {
            pm = meshes;
        } else {
            const uint32_t bit = pass - 1;
            uint32_t gid = 0;
            for (const MeshIn& m : meshes) {
                MeshIn u;
                for (size_t k = 0; k < m.idx.size(); ++k) {
                    const uint32_t face = gid + (uint32_t)(k / 3);
                    const bool set = (face >> bit) & 1u;
                    const float* p = &m.pos[(size_t)m.idx[k] * 3];
                    u.pos.insert(u.pos.end(), p, p + 3);
                    const float n[3] = {set ? 0.f : 1.f, 0.f, set ? 1.f : 0.f};
                    u.nrm.insert(u.nrm.end(), n, n + 3);
                    u.idx.push_back((uint32_t)k);
                }
                gid += (uint32_t)(m.idx.size() / 3);
                pm.push_back(std::move(u));
            }
        }
        Beam::sptr<Beam::IScene> scene = Beam::IScene::create();
        std::vector<Beam::sptr<Beam::IMesh>> keep;
        for (const MeshIn& m : pm) {
            Beam::sptr<Beam::IMesh> mesh = Beam::IMesh::create();
            const uint32_t nv = (uint32_t)(m.pos.size() / 3);
            must(mesh->setIndices(m.idx.data(), (uint32_t)m.idx.size()), "setIndices");
            must(mesh->setVertexData(m.pos.data(), nv, 3, Beam::VERTEX_DATA_POSITION), "setVertexData(POSITION)");
            must(mesh->setVertexData(m.nrm.data(), nv, 3, Beam::VERTEX_DATA_NORMAL), "setVertexData(NORMAL)");
            scene->addMesh(mesh);
            keep.push_back(mesh);
        }
        scene->updateGPUScene();
        std::fflush(stdout);
        Beam::sptr<Beam::ICamera> camera = Beam::ICamera::create();
        must(camera->setInitialRays(w, h, cam[0], cam[1], cam[2], cam[3], cam[4]), "setInitialRays");
        for (const View& v : views) {
            Beam::RenderTarget rt(w, h, w * 4);
            must(rt.lock(), "lock");
            must(camera->traceScene(v.eye, v.orient, scene), "traceScene");
            std::fwrite(g_pixels.data(), 4, g_pixels.size(), out);
            must(rt.unlock(), "unlock");
        }
    }
    std::printf("== ref_frame done\n");
    std::fclose(out);
    return 0;
}
