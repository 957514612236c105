// Beam.h — the reference's C++ host API (Raytracer/Beam.h:32-72), rebuilt header-only over the
// C ABI of libbeam_hip.so (include/beam_c.h). A program written against the reference's
// IScene / IMesh / ICamera / IRenderTarget compiles against this header with two changes:
//   * IRenderTarget::registerGLTBO (GL interop) is replaced by IRenderTarget::createOffscreen;
//   * the device is chosen with Beam::setDevice(n) (default: the BM_DEVICE env var, else 0)
//     instead of cudaSetDevice (TestProgram/Program.cpp:122-124);
//   * Beam::setDevices({d0, d1, ...}) (or env BM_DEVICES="0,1,2,3") renders every frame on several
//     GPUs: scenes are replicated, screen bands dealt round-robin, the frame gathered on d0.
// Error codes, vertex slots, the "current render target" set by lock() (RenderTarget.cpp:53-88)
// and the asynchronous launch behaviour are the reference's. Beam::sync() waits for the device.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../beam_c.h"

namespace Beam {

using i32 = int32_t;
using i64 = int64_t;
using u32 = uint32_t;
using u64 = uint64_t;
template <typename T>
using sptr = std::shared_ptr<T>;
template <typename T>
using wptr = std::weak_ptr<T>;
template <typename T>
using Array = std::vector<T>;

constexpr u32 ERROR_ALL_FINE = BM_ERROR_ALL_FINE;
constexpr u32 ERROR_NO_VERTICES = BM_ERROR_NO_VERTICES;
constexpr u32 ERROR_INVALID_PARAMETER = BM_ERROR_INVALID_PARAMETER;
constexpr u32 ERROR_GPU_ALLOC_FAIL = BM_ERROR_GPU_ALLOC_FAIL;
constexpr u32 ERROR_INVALID_FORMAT = BM_ERROR_INVALID_FORMAT;
constexpr u32 ERROR_RT_CAM_MISMATCH = BM_ERROR_RT_CAM_MISMATCH;
constexpr u32 ERROR_UNLOCK_FIRST = BM_ERROR_UNLOCK_FIRST;
constexpr u32 ERROR_LOCK_FIRST = BM_ERROR_LOCK_FIRST;
constexpr u32 ERROR_NO_RENDER_TARGET = BM_ERROR_NO_RENDER_TARGET;
constexpr u32 ERROR_DEVICE = BM_ERROR_DEVICE;
constexpr u32 ERROR_NOT_BUILT = BM_ERROR_NOT_BUILT;

constexpr u32 VERTEX_DATA_POSITION = 0;
constexpr u32 VERTEX_DATA_NORMAL = 1;
constexpr u32 VERTEX_DATA_UV1 = 2;
constexpr u32 VERTEX_DATA_UV2 = 3;
constexpr u32 VERTEX_DATA_TANGENT = 4;
constexpr u32 VERTEX_DATA_BITANGENT = 5;
constexpr u32 VERTEX_DATA_EXTRA1 = 6;
constexpr u32 VERTEX_DATA_EXTRA2 = 7;
constexpr u32 VERTEX_DATA_EXTRA3 = 8;
constexpr u32 VERTEX_DATA_EXTRA4 = 9;
constexpr u32 VERTEX_DATA_COUNT = 10;

namespace detail {
inline uint32_t& flags_slot() {  // BM_OPT_* for the context created on first use
    static uint32_t f = (std::getenv("BM_REFERENCE_KD") && std::atoi(std::getenv("BM_REFERENCE_KD"))) ? BM_OPT_REFERENCE_KD
                                                                                                   : 0u;
    return f;
}
struct MultiDevice {  // bm_options multi-GPU fields for the context created on first use
    std::vector<int> devices;
    u32 band_height = 0, gather = BM_GATHER_AUTO;
};
inline MultiDevice& multi_slot() {
    static MultiDevice m = [] {
        MultiDevice d;
        if (const char* e = std::getenv("BM_DEVICES")) {  // "0,1,2,3"
            for (const char* p = e; *p;) {
                char* end = nullptr;
                const long v = std::strtol(p, &end, 10);
                if (end == p) break;
                d.devices.push_back((int)v);
                p = *end == ',' ? end + 1 : end;
            }
        }
        return d;
    }();
    return m;
}
struct Context {
    bm_context* h = nullptr;
    explicit Context(int device) {
        bm_options o{};
        o.device = device;
        o.flags = flags_slot();
        const MultiDevice& m = multi_slot();
        if (m.devices.size() > BM_MAX_DEVICES) throw std::runtime_error("Beam: at most 8 devices");
        o.num_devices = (uint32_t)m.devices.size();
        for (size_t i = 0; i < m.devices.size(); ++i) o.devices[i] = m.devices[i];
        o.band_height = m.band_height;
        o.gather = m.gather;
        if (bm_context_create(&o, &h) != BM_ERROR_ALL_FINE) throw std::runtime_error("Beam: no usable HIP device");
    }
    ~Context() { bm_context_destroy(h); }
};
inline int& device_slot() {
    static int d = std::getenv("BM_DEVICE") ? std::atoi(std::getenv("BM_DEVICE")) : 0;
    return d;
}
inline sptr<Context>& context_slot() {
    static sptr<Context> c;
    return c;
}
inline bm_context* ctx() {
    auto& c = context_slot();
    if (!c) c = std::make_shared<Context>(device_slot());
    return c->h;
}
}  // namespace detail

// Select the device before the first Beam object is created.
inline void setDevice(int device) { detail::device_slot() = device; }
// Render on several devices (1..8; repeats allowed: a one-GPU rehearsal): objects replicated on
// each, screen bands of bandHeight rows (0 = 16) dealt round-robin, the frame gathered on
// devices[0] by `gather` (BM_GATHER_AUTO / _PEER / _RCCL). Before the first Beam object.
inline void setDevices(const std::vector<int>& devices, u32 bandHeight = 0, u32 gather = BM_GATHER_AUTO) {
    detail::multi_slot() = detail::MultiDevice{devices, bandHeight, gather};
}
inline u32 numDevices() { return bm_context_num_devices(detail::ctx()); }
// Reference mode (BM_OPT_REFERENCE_KD; env BM_REFERENCE_KD=1): scenes build the reference's kd-tree
// and traceScene returns its first-hit-leaf answer, pixel for pixel. Before the first Beam object.
inline void setReferenceMode(bool on) {
    if (on) detail::flags_slot() = (detail::flags_slot() | BM_OPT_REFERENCE_KD) & ~BM_OPT_REFERENCE_HASH;
    else detail::flags_slot() &= ~BM_OPT_REFERENCE_KD;
}
// Hashed-grid mode (BM_OPT_REFERENCE_HASH): the reference's alternative accelerator (Hash.cu, built
// there with TREE_TYPE==HASH, SceneHash.cpp) — a comparison study. Before the first Beam object.
inline void setHashGridMode(bool on) {
    if (on) detail::flags_slot() = (detail::flags_slot() | BM_OPT_REFERENCE_HASH) & ~BM_OPT_REFERENCE_KD;
    else detail::flags_slot() &= ~BM_OPT_REFERENCE_HASH;
}
// A column-major 4x4 (16 floats, glm::mat4's memory layout: element (r, c) at m[4*c + r]) as the 12-float
// row-major 3x4 transform of IScene::addInstance; the fourth row is dropped (an affine matrix has 0,0,0,1 there).
inline void xformFromColumnMajor4x4(const float colMajor16[16], float xformOut[12]) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) xformOut[4 * r + c] = colMajor16[4 * c + r];
}
// The map an instance's normals go through: the cofactor matrix of xform's linear part, row-major 3x3.
inline u32 normalMatrix(const float xform[12], float out9[9]) { return (u32)bm_xform_normal_matrix(xform, out9); }
inline u32 sync() { return (u32)bm_sync(detail::ctx()); }
inline std::string lastError() { return bm_last_error_string(detail::ctx()); }

class IRenderTarget {
   public:
    // Offscreen device render target: planes packed (0x00RRGGBB, pitch honoured), triangle id, t.
    static sptr<IRenderTarget> createOffscreen(u32 width, u32 height, u32 pitch = 0) {
        bm_rt* h = nullptr;
        if (bm_rt_create_offscreen(detail::ctx(), width, height, pitch, &h) != BM_ERROR_ALL_FINE) return nullptr;
        return sptr<IRenderTarget>(new IRenderTarget(h));
    }
    // GL interop is not part of this build (offscreen framebuffers only).
    static sptr<IRenderTarget> registerGLTBO(u32, u32, u32, u32) { return nullptr; }
    ~IRenderTarget() {
        if (current() == this) current() = nullptr;
        bm_rt_destroy(h_);
    }
    void* buffer() const { return bm_rt_buffer(h_); }
    template <class T>
    T* buffer() const {
        return reinterpret_cast<T*>(buffer());
    }
    u32 pitch() const { return bm_rt_pitch(h_); }
    u32 width() const { return bm_rt_width(h_); }
    u32 height() const { return bm_rt_height(h_); }
    u32 lock() {
        const u32 e = (u32)bm_rt_lock(h_);
        if (e == ERROR_ALL_FINE) current() = this;
        return e;
    }
    u32 unlock() {
        const u32 e = (u32)bm_rt_unlock(h_);
        if (e == ERROR_ALL_FINE && current() == this) current() = nullptr;
        return e;
    }
    // Host readback (synchronous); any pointer may be null.
    u32 read(u32* packed, u32* triId = nullptr, float* t = nullptr, float* rgb = nullptr) {
        return (u32)bm_rt_read(h_, packed, triId, t, rgb);
    }
    u32 readShadow(unsigned char* out) { return (u32)bm_rt_read_shadow(h_, out); }
    u32 savePPM(const char* path) { return (u32)bm_rt_save_ppm(h_, path); }
    // frames in flight: this target's traces/readbacks on its own HIP stream (nullptr: the context's)
    u32 setStream(void* stream) { return (u32)bm_rt_set_stream(h_, stream); }
    static IRenderTarget*& current() {  // RenderTarget::m_RT (RenderTarget.cpp:85-93)
        static IRenderTarget* rt = nullptr;
        return rt;
    }
    bm_rt* handle() const { return h_; }

   private:
    explicit IRenderTarget(bm_rt* h) : h_(h) {}
    bm_rt* h_;
};

class IScene;

class IMesh {
   public:
    static sptr<IMesh> create() {
        bm_mesh* h = nullptr;
        if (bm_mesh_create(detail::ctx(), &h) != BM_ERROR_ALL_FINE) return nullptr;
        return sptr<IMesh>(new IMesh(h));
    }
    ~IMesh() { bm_mesh_destroy(h_); }
    u32 setVertexData(const float* vertices, u32 numVertices, u32 numComponents, u32 slotId, bool asyncCopy = false) {
        (void)asyncCopy;
        return (u32)bm_mesh_set_vertex_data(h_, vertices, numVertices, numComponents, slotId);
    }
    u32 setIndices(const u32* indices, u32 numIndices, bool asyncCopy = false) {
        (void)asyncCopy;
        return (u32)bm_mesh_set_indices(h_, indices, numIndices);
    }
    // Device-side deformation (beam_c.h, "device-side mesh deformation"): vertex data from device memory and a
    // slot's read-back, both enqueued on the context stream without a host wait, and smooth vertex normals
    // recomputed from the positions and indices.
    u32 setVertexDataDevice(const float* verticesDev, u32 numVertices, u32 numComponents, u32 slotId) {
        return (u32)bm_mesh_set_vertex_data_device(h_, verticesDev, numVertices, numComponents, slotId);
    }
    u32 copyVertexDataDevice(u32 slotId, float* outDev, u32 numVertices, u32 numComponents) const {
        return (u32)bm_mesh_copy_vertex_data_device(h_, slotId, outDev, numVertices, numComponents);
    }
    u32 computeNormals(bool normalize = true) {
        return (u32)bm_mesh_compute_normals(h_, normalize ? BM_NORMALS_NORMALIZE : 0u);
    }
    wptr<IScene> scene() const { return {}; }
    bm_mesh* handle() const { return h_; }

   private:
    explicit IMesh(bm_mesh* h) : h_(h) {}
    bm_mesh* h_;
};

class IScene {
   public:
    static sptr<IScene> create() {
        bm_scene* h = nullptr;
        if (bm_scene_create(detail::ctx(), &h) != BM_ERROR_ALL_FINE) return nullptr;
        return sptr<IScene>(new IScene(h));
    }
    ~IScene() { bm_scene_destroy(h_); }
    void addMesh(const sptr<IMesh>& mesh) {
        if (bm_scene_add_mesh(h_, mesh->handle()) == BM_ERROR_ALL_FINE) meshes_.push_back(mesh);
    }
    void removeMesh(const IMesh& mesh) {
        bm_scene_remove_mesh(h_, mesh.handle());
        for (auto it = meshes_.begin(); it != meshes_.end(); ++it)
            if (it->get() == &mesh) {
                meshes_.erase(it);
                break;
            }
    }
    // Rebuilds the BVH (asynchronous, like the reference's launches).
    void updateGPUScene() { bm_scene_build(h_, nullptr); }
    u32 updateGPUScene(bm_build_stats* stats) { return (u32)bm_scene_build(h_, stats); }
    // Extension: refit-only update after vertex data changed (same meshes and triangle counts).
    u32 refitGPUScene(bm_build_stats* stats = nullptr) { return (u32)bm_scene_refit(h_, stats); }
    // Extension: ray queries over n rays in device memory (bm_scene_trace_rays; asynchronous on the
    // context stream). traceRays: the closest hit within each ray's tmax; occluded: one byte per ray,
    // 1 when anything lies on the segment origin -> origin + dir. flags: 0 or the filter bits
    // BM_RAYS_CULL_* / BM_RAYS_PAD_* (face culling; pad as a triangle to skip, a tmin or a ray mask).
    u32 traceRays(const bm_ray* deviceRays, u32 n, bm_hit* deviceHits, u32 flags = 0) {
        return (u32)bm_scene_trace_rays(h_, deviceRays, n, BM_RAYS_CLOSEST, flags, deviceHits);
    }
    u32 occluded(const bm_ray* deviceRays, u32 n, uint8_t* deviceOut, u32 flags = 0) {
        return (u32)bm_scene_trace_rays(h_, deviceRays, n, BM_RAYS_ANY_HIT, flags, deviceOut);
    }
    // Extension: the k nearest hits of each ray in (t, id) order, k records per ray (bm_scene_trace_rays_multi;
    // asynchronous on the context stream). deviceCounts (optional): the records that are hits; with
    // flags = BM_MULTI_COUNT_ALL (deviceCounts required, k may be 0) every crossing within tmax. The filter bits
    // of traceRays combine with it.
    u32 traceRaysMulti(const bm_ray* deviceRays, u32 n, u32 k, bm_hit* deviceHits, uint32_t* deviceCounts = nullptr,
                       u32 flags = 0) {
        return (u32)bm_scene_trace_rays_multi(h_, deviceRays, n, k, flags, deviceHits, deviceCounts);
    }
    // Extension: the meshes' vertex slots interpolated at n hit records in device memory, up to
    // BM_ATTR_MAX_REQS requests per call (bm_scene_hit_attributes; asynchronous on the context stream).
    u32 hitAttributes(const bm_hit* deviceHits, u32 n, const bm_attr_req* reqs, u32 numReqs) {
        return (u32)bm_scene_hit_attributes(h_, deviceHits, n, reqs, numReqs);
    }
    // Extension: the nearest triangle to each of n points in device memory (bm_scene_closest_points;
    // asynchronous on the context stream): distance, barycentrics and triangle id as bm_hit records, which
    // hitAttributes turns into the closest point (BM_VERTEX_DATA_POSITION), its normal or its mesh and face.
    u32 closestPoints(const bm_point* devicePoints, u32 n, bm_hit* deviceHits) {
        return (u32)bm_scene_closest_points(h_, devicePoints, n, 0, deviceHits);
    }
    // Extension: the k nearest triangles within each point's rmax in (distance, id) order, k records per point
    // (bm_scene_closest_points_multi; asynchronous on the context stream). deviceCounts (optional): the records
    // written; with flags = BM_MULTI_COUNT_ALL (deviceCounts required, k may be 0) every triangle within rmax.
    u32 closestPointsMulti(const bm_point* devicePoints, u32 n, u32 k, u32 flags, bm_hit* deviceHits,
                           uint32_t* deviceCounts = nullptr) {
        return (u32)bm_scene_closest_points_multi(h_, devicePoints, n, k, flags, deviceHits, deviceCounts);
    }
    // Extension: the first contact of each of n swept spheres in device memory (bm_scene_sweep_spheres;
    // asynchronous on the context stream). mode BM_SWEEP_CLOSEST: deviceOut is bm_hit[n] (t along dir, the
    // contact point's barycentrics and triangle; hitAttributes gives the contact position); BM_SWEEP_ANY:
    // uint8_t[n], whether the sphere touches anything within tmax.
    u32 sweepSpheres(const bm_sweep* deviceSweeps, u32 n, u32 mode, void* deviceOut) {
        return (u32)bm_scene_sweep_spheres(h_, deviceSweeps, n, mode, 0, deviceOut);
    }
    // Extension: inside or outside, and the signed distance, of each of n points in device memory
    // (bm_scene_signed_distances; asynchronous on the context stream). mode BM_SIGNED_DISTANCE: deviceOut is
    // bm_hit[n], closestPoints' record with the sign bit of t set inside; BM_SIGNED_OCCUPANCY: uint8_t[n].
    // flags: 0 (one sample direction) or BM_SIGNED_VOTE3 (the majority of three). deviceVotes (optional):
    // uint8_t[n], the votes for inside.
    u32 signedDistances(const bm_point* devicePoints, u32 n, u32 mode, u32 flags, void* deviceOut,
                        uint8_t* deviceVotes = nullptr) {
        return (u32)bm_scene_signed_distances(h_, devicePoints, n, mode, flags, deviceOut, deviceVotes);
    }
    // Extension: the triangles that intersect each of n axis-aligned boxes in device memory
    // (bm_scene_overlap_boxes; asynchronous on the context stream). mode BM_BOXES_COUNT: deviceOut is
    // uint32_t[n]; BM_BOXES_ANY: uint8_t[n]; BM_BOXES_LIST: the ids go to deviceIds at the segments of
    // deviceOffsets (n + 1 ascending values), the counts to deviceOut unless it is null.
    u32 overlapBoxes(const bm_box* deviceBoxes, u32 n, u32 mode, void* deviceOut,
                     const uint32_t* deviceOffsets = nullptr, uint32_t* deviceIds = nullptr) {
        return (u32)bm_scene_overlap_boxes(h_, deviceBoxes, n, mode, 0, deviceOut, deviceOffsets, deviceIds);
    }
    // Extension: the scene triangles that intersect each of n query triangles in device memory
    // (bm_scene_overlap_triangles; asynchronous on the context stream). Modes and outputs as overlapBoxes
    // with BM_TRIS_*; flags 0 or BM_TRIS_PAD_SKIP_TRI (pad0 of each record: an id that is never reported).
    u32 overlapTriangles(const bm_tri* deviceTris, u32 n, u32 mode, void* deviceOut,
                         const uint32_t* deviceOffsets = nullptr, uint32_t* deviceIds = nullptr, u32 flags = 0) {
        return (u32)bm_scene_overlap_triangles(h_, deviceTris, n, mode, flags, deviceOut, deviceOffsets, deviceIds);
    }
    // Extension: the triangles each of n planes in device memory crosses, and their cut segments
    // (bm_scene_section_planes; asynchronous on the context stream). mode BM_PLANES_COUNT: deviceOut is
    // uint32_t[n]; BM_PLANES_ANY: uint8_t[n]; BM_PLANES_LIST: slot j of plane i goes to deviceIds and/or
    // deviceSegments (at least one) at deviceOffsets[i] + j (n + 1 ascending values), the counts to deviceOut
    // unless it is null. On a closed mesh the segments chain into closed loops by equality of their endpoints.
    u32 sectionPlanes(const bm_plane* devicePlanes, u32 n, u32 mode, void* deviceOut,
                      const uint32_t* deviceOffsets = nullptr, uint32_t* deviceIds = nullptr,
                      bm_segment* deviceSegments = nullptr) {
        return (u32)bm_scene_section_planes(h_, devicePlanes, n, mode, 0, deviceOut, deviceOffsets, deviceIds,
                                            deviceSegments);
    }
    // Extension: instance transforms (include/beam_c.h, "instance transforms"). xform: 12 floats, row-major
    // 3x4 (xformFromColumnMajor4x4 converts a glm::mat4's 16 floats). addInstance appends the mesh at that
    // placement and reports the entry's index; setInstanceTransform takes effect at the next updateGPUScene
    // or refitGPUScene; removeInstance erases the entry at index, plain or instance.
    u32 addInstance(const sptr<IMesh>& mesh, const float xform[12], u32* index = nullptr) {
        if (!mesh) return ERROR_INVALID_PARAMETER;
        const u32 e = (u32)bm_scene_add_instance(h_, mesh->handle(), xform, index);
        if (e == ERROR_ALL_FINE) meshes_.push_back(mesh);
        return e;
    }
    u32 addInstance(IMesh* mesh, const float xform[12], u32* index = nullptr) {  // the caller keeps the mesh alive
        return (u32)bm_scene_add_instance(h_, mesh ? mesh->handle() : nullptr, xform, index);
    }
    u32 setInstanceTransform(u32 index, const float xform[12]) {
        return (u32)bm_scene_set_instance_transform(h_, index, xform);
    }
    u32 instanceTransform(u32 index, float xformOut[12]) const {
        return (u32)bm_scene_get_instance_transform(h_, index, xformOut);
    }
    u32 removeInstance(u32 index) { return (u32)bm_scene_remove_instance(h_, index); }
    // Extension: the 32-bit visibility mask of the entry at index, plain or instance (default 0xFFFFFFFF), which
    // BM_RAYS_PAD_MASK ray queries test against each ray's mask; no rebuild needed (bm_scene_set_entry_mask).
    u32 setEntryMask(u32 index, u32 mask) { return (u32)bm_scene_set_entry_mask(h_, index, mask); }
    u32 getEntryMask(u32 index, u32* maskOut) const { return (u32)bm_scene_get_entry_mask(h_, index, maskOut); }
    bm_scene* handle() const { return h_; }

   private:
    explicit IScene(bm_scene* h) : h_(h) {}
    bm_scene* h_;
    Array<sptr<IMesh>> meshes_;
};

class ICamera {
   public:
    static sptr<ICamera> create() {
        bm_camera* h = nullptr;
        if (bm_camera_create(detail::ctx(), &h) != BM_ERROR_ALL_FINE) return nullptr;
        return sptr<ICamera>(new ICamera(h));
    }
    ~ICamera() { bm_camera_destroy(h_); }
    u32 setInitialRays(u32 width, u32 height, float left = -1, float right = 1, float top = 1, float bottom = -1,
                       float zoom = 1) {
        return (u32)bm_camera_set_initial_rays(h_, width, height, left, right, top, bottom, zoom);
    }
    u32 clear(u32 value) {
        IRenderTarget* rt = IRenderTarget::current();
        if (!rt) return ERROR_NO_RENDER_TARGET;
        return (u32)bm_rt_clear(rt->handle(), value);
    }
    u32 traceScene(const float* eye3, const float* orient3x3, sptr<IScene>& scene) {
        IRenderTarget* rt = IRenderTarget::current();
        if (!rt) return ERROR_NO_RENDER_TARGET;
        if (!scene) return ERROR_INVALID_PARAMETER;
        return (u32)bm_camera_trace(h_, eye3, orient3x3, scene->handle(), rt->handle());
    }
    // Extension (no reference counterpart): traceScene plus one any-hit shadow ray per hit toward
    // a point light; the current render target's shadow plane (readShadow) gets 1 = shadowed.
    u32 traceSceneShadow(const float* eye3, const float* orient3x3, sptr<IScene>& scene, const float* light3) {
        IRenderTarget* rt = IRenderTarget::current();
        if (!rt) return ERROR_NO_RENDER_TARGET;
        if (!scene) return ERROR_INVALID_PARAMETER;
        return (u32)bm_camera_trace_shadow(h_, eye3, orient3x3, scene->handle(), rt->handle(), light3);
    }

   private:
    explicit ICamera(bm_camera* h) : h_(h) {}
    bm_camera* h_;
};

}  // namespace Beam
