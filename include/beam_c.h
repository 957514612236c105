/*
 * beam_c.h — C ABI of the MI355X-native Beam primary-ray path (libbeam_hip.so).
 *
 * Drop-in boundary for the reference's hot path. The reference splits its host API
 * (Raytracer/Beam.h:32-72, C++ classes) from its device entry points (extern "C" declarations at
 * Raytracer/SceneTree.cpp:11-35 and Raytracer/Camera.cpp:16-19), and those pass glm types by value
 * and by reference, so they are not a real C ABI. Everything here is POD: opaque handles, plain
 * pointers, sizes and int32 error codes. include/beam/Beam.h rebuilds the reference's C++
 * interface classes on top of it; INTEGRATION.md shows the ctypes / C++ bindings.
 *
 * Threading and streams: one host thread per context. Every device operation is enqueued on the
 * context's HIP stream (its own, or one supplied in bm_options) and returns without waiting,
 * like the reference's launches on the legacy default stream; bm_sync() waits. Mesh uploads copy
 * from the caller's host memory before returning (the reference's synchronous cudaMemcpy,
 * DeviceBuffer.cpp:44-58). Handles must be destroyed before their context.
 *
 * Errors: the reference's u32 codes (Raytracer/Beam.h:8-16) plus BM_ERROR_DEVICE for any HIP
 * failure (the reference calls exit(1) from CUDA_CALL, CudaComon.cuh:59-68) and
 * BM_ERROR_NOT_BUILT for tracing a scene that has no current build.
 * bm_last_error_string() describes the last failure on a context.
 */
#ifndef BEAM_C_H
#define BEAM_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM_ERROR_ALL_FINE 0
#define BM_ERROR_NO_VERTICES 1
#define BM_ERROR_INVALID_PARAMETER 2
#define BM_ERROR_GPU_ALLOC_FAIL 3
#define BM_ERROR_INVALID_FORMAT 4
#define BM_ERROR_RT_CAM_MISMATCH 5
#define BM_ERROR_UNLOCK_FIRST 6
#define BM_ERROR_LOCK_FIRST 7
#define BM_ERROR_NO_RENDER_TARGET 8
#define BM_ERROR_DEVICE 9
#define BM_ERROR_NOT_BUILT 10

/* Vertex data slots (Raytracer/Beam.h:19-29). */
#define BM_VERTEX_DATA_POSITION 0
#define BM_VERTEX_DATA_NORMAL 1
#define BM_VERTEX_DATA_UV1 2
#define BM_VERTEX_DATA_UV2 3
#define BM_VERTEX_DATA_TANGENT 4
#define BM_VERTEX_DATA_BITANGENT 5
#define BM_VERTEX_DATA_EXTRA1 6
#define BM_VERTEX_DATA_EXTRA2 7
#define BM_VERTEX_DATA_EXTRA3 8
#define BM_VERTEX_DATA_EXTRA4 9
#define BM_VERTEX_DATA_COUNT 10

/* Framebuffer values (Raytracer/BuildTree.cu:486-496; pixel format 0x00RRGGBB, GLinterop.h). */
#define BM_MISS_PACKED 0x0000FF00u
#define BM_NO_TRIANGLE 0xFFFFFFFFu

typedef struct bm_context bm_context;
typedef struct bm_mesh bm_mesh;
typedef struct bm_scene bm_scene;
typedef struct bm_camera bm_camera;
typedef struct bm_rt bm_rt;

#define BM_MAX_DEVICES 8
#define BM_COMM_ID_BYTES 128

typedef struct bm_options {
    int32_t device;      /* HIP device ordinal (the reference picks the last one, Program.cpp:122-124) */
    void* stream;        /* hipStream_t to enqueue on, or NULL for a stream owned by the context */
    uint32_t leaf_size;  /* BVH leaf collapse size, 1..16 (0 = default 4) */
    uint32_t flags;      /* BM_OPT_* bits */
    /* ---- multi-GPU; all zero = one device. The reference has no device control
     * beyond cudaSetDevice(count-1) in its demo (TestProgram/Program.cpp:121-124). ---------------- */
    /* One process, several devices: devices[0..num_devices) (1..8; 0 = `device` alone). Every mesh,
     * scene and camera created on the context is replicated on each device (the build is
     * deterministic, so the replicas are bit-identical); a trace deals the frame's screen bands
     * (band_height rows, band b -> device b % n) to the devices and gathers them into the render
     * target, which lives on devices[0] (the root; `stream` applies to it). A device may be listed
     * more than once (several band streams sharing one GPU: a one-GPU rehearsal of the n-way path). */
    uint32_t num_devices;
    int32_t devices[BM_MAX_DEVICES];
    uint32_t band_height;    /* rows per screen band, 0 = 16 */
    uint32_t gather;         /* BM_GATHER_* transport of the band buffers to the root */
    uint32_t gather_planes;  /* 0: the triangle-id plane (+ shadow bytes) travels and the root rebuilds
                                t, |n.z| and the packed colour from it (4 B/pixel, every plane exact);
                                else a BM_PLANE_* mask of planes moved as traced */
    /* Several processes, one device each (e.g. launched by torchrun): rank comm_rank of comm_size
     * (0 or 1: no communicator), joined by the RCCL unique id rank 0 made with bm_comm_unique_id and
     * handed to the other ranks by the caller. A trace then covers this rank's bands and gathers
     * every rank's bands into rank 0's render target over RCCL (the render targets of other ranks
     * are left unwritten); builds are replicated per rank as above. */
    int32_t comm_rank;
    int32_t comm_size;
    uint8_t comm_id[BM_COMM_ID_BYTES];
} bm_options;

/* Gather transports (bm_options.gather). */
#define BM_GATHER_AUTO 0u  /* PEER for one process, RCCL between processes */
#define BM_GATHER_PEER 1u  /* each device writes its bands into the root's planes over xGMI (peer
                              access; a kernel on the source device, no staging copy) */
#define BM_GATHER_RCCL 2u  /* one RCCL communicator over the devices (ncclCommInitAll): grouped
                              ncclSend/ncclRecv into root staging buffers, then one scatter kernel
                              on the root. A device list that repeats a device (RCCL refuses two
                              ranks on one GPU) gets one single-rank communicator instead (unique id
                              + ncclCommInitRank) and every band travels as a send/recv to itself:
                              the same staging and scatter, rehearsed on one GPU */
/* bm_context_gather's answer for that single-rank rehearsal (never an option value). */
#define BM_GATHER_RCCL_LOOPBACK 3u
/* Planes a multi-device trace gathers (bm_options.gather_planes). */
#define BM_PLANE_PACKED 1u  /* the reference's framebuffer, 0x00RRGGBB */
#define BM_PLANE_TRI_ID 2u
#define BM_PLANE_T 4u
#define BM_PLANE_NZ 8u      /* |n.z| of the shading normal (rgb readback) */
#define BM_PLANE_SHADOW 16u /* u8 shadow plane of shadow traces */

/* Enqueue on the legacy default (null) stream, e.g. torch's default stream, whose handle is 0. */
#define BM_OPT_NULL_STREAM 1u
/* Shadow rays as a separate wavefront pass over a device queue of the hit pixels (compacted with
 * wave64 ballots) instead of fused into the primary kernel; same results, a compaction study. */
#define BM_OPT_SHADOW_QUEUE 2u
/* Build BVH2 (binary, 64-B records) instead of the default BVH4 (128-B records, every other level
 * of the binary tree collapsed). Same frames; fewer, wider node steps with BVH4. */
#define BM_OPT_BVH2 4u
/* Build BVH8 (256-B records, three binary levels per node, collapsed from the BVH2 records) and
 * trace it with ray quads (two children per lane): a third fewer node steps, but each step costs
 * more than it saves — measured 12-16 % slower than the default BVH4. Compiled into
 * A/B builds only (bm_version() ending in "+ab", tools/build_ab.py); the product library rejects the
 * flag with BM_ERROR_INVALID_PARAMETER. Primary and fused shadow rays with the default trace (no
 * shadow queue, no trace variants); excludes BM_OPT_BVH2. */
#define BM_OPT_BVH8 32u
/* Reference mode: scenes build the reference's own sparse kd-tree (world box [-30,30]³, SAT
 * insertion, 31 levels, 256-face leaves; BuildTree.cu:154-362) and traces march it with the
 * first-hit-leaf early-out (BuildTree.cu:367-499), so every pixel equals the reference framebuffer,
 * including the pixels where that early-out returns a farther triangle than the closest hit.
 * Full-frame bm_camera_trace only (no bands, shadows, refit or export; bm_camera_trace_counters
 * returns node records visited, face tests and hits; bm_camera_trace_profile a wave per 8x8 tile).
 * One device only. */
#define BM_OPT_REFERENCE_KD 8u
/* Hashed-grid mode: the reference's alternative accelerator (Raytracer/Hash.cu, compiled there only
 * with TREE_TYPE==HASH): 0.03 cells hashed into 65,536 buckets by Fletcher-16, every
 * SAT-accepted cell of a triangle's AABB (the insert loop's row reset fixed), 256 faces per bucket;
 * the march steps cell by cell from the eye (at most 400) and returns the closest hit of the first
 * bucket with any hit, collisions included. Full-frame bm_camera_trace only; excludes
 * BM_OPT_REFERENCE_KD. A comparison study, not a renderer: see DESIGN.md §7. */
#define BM_OPT_REFERENCE_HASH 16u

/* bm_build_stats.sort_path: how the build sorted its Morton keys. */
#define BM_SORT_LSD 1u      /* three 10-bit LSD one-sweep passes */
#define BM_SORT_MSD 2u      /* the top digit first, then every bucket in one workgroup's LDS */
#define BM_SORT_MSD_SKEW 3u /* the top-digit histogram showed a bucket too large for LDS: the same
                               build sorted with the LSD passes instead (decided on the device) */
/* reference mode (BM_OPT_REFERENCE_KD) reports its (leaf, face) pair sort: BM_SORT_LSD (four 10-bit
 * passes over the 31-bit leaf paths) or BM_SORT_KD_RANKED (three: the last on the rank of the paths'
 * top 11 bits among those present, when at most 1,024 are) — the same order either way */
#define BM_SORT_KD_RANKED 4u
typedef struct bm_build_stats {
    uint32_t num_meshes;
    uint32_t num_tris;
    uint32_t num_records;  /* node record slots (bvh_width 2: 64 B each, 4: 128 B each) */
    uint32_t leaf_size;
    float build_ms;        /* device time gather+bounds+Morton+sort+emit+refit+pack (hipEvents) */
    uint32_t bvh_width;    /* 4 (default), 2 (BM_OPT_BVH2) or 8 (BM_OPT_BVH8, A/B builds only) */
    uint32_t sort_path;    /* the sort this build ran: BM_SORT_* (0 for refits and the hashed grid) */
    uint32_t fused_front;  /* always 0 (round 5: k_front removed; kept for ABI stability) */
} bm_build_stats;

/* ---- context ------------------------------------------------------------------------------ */
int32_t bm_context_create(const bm_options* opts, bm_context** out);
void bm_context_destroy(bm_context* ctx);
int32_t bm_sync(bm_context* ctx);
const char* bm_last_error_string(const bm_context* ctx);
void* bm_context_stream(const bm_context* ctx);       /* the hipStream_t work is enqueued on */
const char* bm_version(void);
/* Devices a context spans (1 for single-device contexts; comm_size for multi-process ones). */
uint32_t bm_context_num_devices(const bm_context* ctx);
/* Multi-process gather: rank 0 makes the RCCL unique id (BM_COMM_ID_BYTES bytes) that every rank
 * passes in bm_options.comm_id. BM_ERROR_DEVICE when RCCL (librccl.so.1) cannot be loaded. */
int32_t bm_comm_unique_id(uint8_t* id);
/* BM_ERROR_ALL_FINE when RCCL (librccl.so.1) resolves in this process, else BM_ERROR_DEVICE: the
 * check every rank makes before any rank enters the collective communicator start. */
int32_t bm_comm_available(void);
/* The transport a multi-device context resolved (BM_GATHER_PEER, BM_GATHER_RCCL or
 * BM_GATHER_RCCL_LOOPBACK); 0 for single-device contexts. */
uint32_t bm_context_gather(const bm_context* ctx);

/* Split start of a multi-process context: create a plain single-device context on every rank
 * first (bm_options without comm_*; band_height and gather_planes are kept for later), let the
 * ranks agree that every one of them has one, then join the RCCL communicator here (the
 * collective ncclCommInitRank). A rank whose device setup fails therefore never leaves the others
 * blocked inside the collective. Needs a context with no devices list, no peers and no render
 * targets yet; size >= 2. Meshes, scenes and cameras made afterwards are this rank's replicas. */
int32_t bm_context_start_comm(bm_context* ctx, int32_t rank, int32_t size, const uint8_t* comm_id);

/* ---- tuning parameters ----------------------------------------------------------------------
 * Measurement and test hooks of the kernels' schedules (the reference's configuration is
 * compile-time only, Types.h:8-13 and BuildTree.cuh:11-21; this library reads nothing from the
 * environment). Per context, set before the work they affect; -1 restores the library default.
 * The defaults are the measured-best settings. BM_ERROR_INVALID_PARAMETER for an
 * unknown key or a value the key does not accept. */
#define BM_PARAM_TRACE_VARIANT 0      /* trace kernel variant (bm_internal.h TraceVariant; A/B builds add more) */
#define BM_PARAM_TRACE_SCHED 1        /* quad tile order: 0 static, 1 screen-order dynamic, 2 cost-ordered */
#define BM_PARAM_TRACE_SCRAMBLE 2     /* lane-per-ray variants: scrambled static tile order */
#define BM_PARAM_TRACE_PRIO_AFTER 3   /* steps before a long-running wave raises its priority */
#define BM_PARAM_TRACE_PRIO_LEVEL 4   /* that priority (0-3) */
#define BM_PARAM_TRACE_REFILL_MIN 5   /* quad-fetch variant: idle quads that trigger a refill */
#define BM_PARAM_CULL_TILES 6         /* compacted trace: 8x8 tiles per culling workgroup region (at most 2^16) */
#define BM_PARAM_TRACE_AUTO_COMPACT 7 /* 0: never switch sparse in-flight views to cull + compacted quads */
#define BM_PARAM_TRACE_GRID 8         /* cap of the persistent trace grid (workgroups) */
#define BM_PARAM_READBACK_SYNC 9      /* 1: mid-build count readbacks by copy + stream sync (A/B) */
#define BM_PARAM_KD_QUEUE_CAP 10      /* reference-mode build: subtree queue items (small: walk-on paths) */
#define BM_PARAM_KD_LQ_CAP 11         /* reference-mode build: LDS queue items per workgroup */
#define BM_PARAM_KD_SPLIT 12          /* reference-mode build: hand-off depth (0: one lane walks all) */
#define BM_PARAM_KD_GRID 13           /* 0: node boxes by the halving recurrence, never the closed form */
#define BM_PARAM_KD_PAIR 14           /* 0: one lane per walk instead of a lane pair */
#define BM_PARAM_KD_TB 15             /* lanes per workgroup of the reference-mode descent (64 or 256) */
#define BM_PARAM_KD_MARCH 16          /* reference-mode march: 3 wave-cooperative leaves, child-box node steps (default), 2 the same with one box per step, 1/0 lane leaves in 64/256-lane groups */
#define BM_PARAM_MSD_MAX_N 17         /* largest scene sorted top digit first (above: three LSD passes) */
#define BM_PARAM_NRM_DEFER 18         /* 0: corner normals gathered by the gather, not the top-digit pass */
#define BM_PARAM_BUCKET_LDS_CAP 19    /* keys a bucket may hold to sort in LDS (0: every bucket via global) */
#define BM_PARAM_MSD_WIDE_N 20        /* above this many triangles the bucket sort runs 1,024-lane workgroups */
#define BM_PARAM_FRONT_MAX_N 21       /* retired (k_front removed in round 5): only 0 / -1 accepted */
#define BM_PARAM_ORIG_LAZY 22         /* test hook: 1 = builds never write the original-order records, so a
                                         multi-device trace rebuilds them lazily (the path a scene built before
                                         bm_context_start_comm takes) */
#define BM_PARAM_KD_MAX_LEAVES 23     /* reference mode: kd leaves a build accepts (default and cap 2^25; a test
                                         hook below): more leave the tree unbuilt and the first trace or kdStats
                                         reports BM_ERROR_GPU_ALLOC_FAIL */
#define BM_PARAM_TRACE_AUTO_PACKET 24 /* 0: never switch dense coherent views to wave packets (BM_PARAM_TRACE_VARIANT 14) */
#define BM_PARAM_KD_TOP_RANK 25 /* 0: reference-mode pair sort in four plain passes (no ranked top digit; A/B) */
#define BM_PARAM_CULL_DEPTH 26 /* compacted trace: record levels k_cull culls by (1, the default: the root record;
                                * 2: the root's entered child records too — fewer queued rays, measured slower) */
#define BM_PARAM_COUNT 27
int32_t bm_context_set_param(bm_context* ctx, uint32_t key, int64_t value);
/* The value set for key, -1 while the library default is in effect; INT64_MIN for an unknown key. */
int64_t bm_context_get_param(const bm_context* ctx, uint32_t key);

/* ---- mesh: IMesh (Beam.h:47-54, Mesh.cpp:30-54) ------------------------------------------ */
int32_t bm_mesh_create(bm_context* ctx, bm_mesh** out);
/* numComponents <= 4; position must have 3; all slots share one vertex count (Mesh.cpp:32-37). */
int32_t bm_mesh_set_vertex_data(bm_mesh* m, const float* data, uint32_t num_vertices,
                                uint32_t num_components, uint32_t slot);
/* num_indices % 3 == 0 (Mesh.cpp:48). */
int32_t bm_mesh_set_indices(bm_mesh* m, const uint32_t* indices, uint32_t num_indices);
void bm_mesh_destroy(bm_mesh* m);

/* ---- device-side mesh deformation: vertex data from device memory, vertex normals ---------
 * For meshes whose vertices are computed on the GPU (cloth, soft bodies, skinning, morph targets): the loop
 * "simulate, upload, refit, query" without a copy to the host and without a host wait. All three calls work
 * on the context stream; make the context on the stream the simulation runs on (bm_options.stream) and the
 * stream orders everything.
 * bm_mesh_set_vertex_data_device: bm_mesh_set_vertex_data with data_dev in device memory of the context's
 *   device: the same parameter rules, checks and error codes. data_dev must not overlap the slot (the library
 *   hands out no slot address, so a buffer of the caller's own never does). The copy is enqueued on the context stream and the call returns without waiting, unless the slot has to
 *   grow (its first upload, or more bytes than any before), which waits as every growing buffer does. Work
 *   enqueued on the context stream before the call sees the old values, work enqueued after it the new ones:
 *   bm_scene_hit_attributes reads mesh slots when its kernel runs and follows that order; builds, refits
 *   and instance transforms read them at build time, so a trace sees new vertices after the next
 *   bm_scene_refit or bm_scene_build. Traces on a render target's own stream (bm_rt_set_stream) are ordered
 *   before the write by an event, not by a host wait. Host and device uploads may be mixed on one mesh;
 *   the host call keeps its synchronous behaviour.
 * bm_mesh_copy_vertex_data_device: the slot's current contents, copied device to device on the context
 *   stream into out_dev (num_vertices * num_components floats); no host wait.
 * bm_mesh_compute_normals: writes the BM_VERTEX_DATA_NORMAL slot (3 components; created when absent, so a
 *   positions-only mesh can then be built) from the position slot and the indices, on the context stream.
 *   The first call after a bm_mesh_set_indices builds the mesh's vertex -> corner table and waits on the
 *   host for that; every later call enqueues one kernel launch and nothing else. The result is defined to
 *   the bit, in float32 with one rounding per operation and no contraction:
 *     for vertex v, take the corners c = 3f + k with idx[c] == v in ascending c (a face naming v twice
 *     contributes twice); with e1 = p[idx[3f+1]] - p[idx[3f]] and e2 = p[idx[3f+2]] - p[idx[3f]] the
 *     corner's face vector is BM_ATTR_GEOM_NORMAL's,
 *       (e1.y*e2.z - e2.y*e1.z,  e1.z*e2.x - e2.z*e1.x,  e1.x*e2.y - e2.x*e1.y),
 *     area-weighted and not normalised; s starts at (0,0,0) and each face vector is added to it component
 *     by component in that order. With BM_NORMALS_NORMALIZE, d = (s.x*s.x + s.y*s.y) + s.z*s.z and, if
 *     d > 0, each component is multiplied by 1.f / sqrtf(d) (BM_ATTR_NORMALIZE's arithmetic: a d of +inf
 *     gives zeros); otherwise s is stored as it is: a vertex without faces, or with degenerate faces only,
 *     gets zeros, and a NaN stays a NaN.
 *   No atomic and no launch shape takes part: the result is the same on every grid and every GPU. A mesh
 *   without indices gets zeros.
 * Multi-device contexts: every replica of the mesh receives an upload by a peer copy ordered after the root's
 *   stream, and computes its own normals. There bm_mesh_set_vertex_data_device and bm_mesh_compute_normals
 *   may wait on the host.
 * Errors:
 *   bm_mesh_set_vertex_data_device   BM_ERROR_INVALID_PARAMETER: a null handle or pointer, no vertices, a
 *                                    slot past BM_VERTEX_DATA_COUNT, components outside 1..4 (positions: 3),
 *                                    a vertex count other than the mesh's.
 *   bm_mesh_copy_vertex_data_device  BM_ERROR_INVALID_PARAMETER: a null handle or pointer, a slot past
 *                                    BM_VERTEX_DATA_COUNT, counts other than the slot's.
 *                                    BM_ERROR_NO_VERTICES: the slot is empty.
 *   bm_mesh_compute_normals          BM_ERROR_INVALID_PARAMETER: a null handle, an unknown flag bit, an index
 *                                    at or past the vertex count. BM_ERROR_NO_VERTICES: no 3-component
 *                                    position slot. */
#define BM_NORMALS_NORMALIZE 1u
int32_t bm_mesh_set_vertex_data_device(bm_mesh* m, const float* data_dev, uint32_t num_vertices,
                                       uint32_t num_components, uint32_t slot);
int32_t bm_mesh_copy_vertex_data_device(const bm_mesh* m, uint32_t slot, float* out_dev,
                                        uint32_t num_vertices, uint32_t num_components);
int32_t bm_mesh_compute_normals(bm_mesh* m, uint32_t flags);

/* ---- scene: IScene (Beam.h:56-63, Scene.cpp, SceneTree.cpp) ------------------------------ */
int32_t bm_scene_create(bm_context* ctx, bm_scene** out);
/* The scene references (does not own) its meshes; keep them alive while it uses them. */
int32_t bm_scene_add_mesh(bm_scene* s, bm_mesh* m);
int32_t bm_scene_remove_mesh(bm_scene* s, bm_mesh* m);
/* updateGPUScene (SceneTree.cpp:70-91): rebuild the acceleration structure from the current
 * meshes; global triangle id = sum of earlier meshes' triangle counts + local face index.
 * stats may be NULL; when given, the call waits for the build to finish to fill build_ms. */
int32_t bm_scene_build(bm_scene* s, bm_build_stats* stats);
/* Refit-only update for animated meshes: the meshes and triangle counts of the
 * last bm_scene_build, new vertex positions/normals (bm_mesh_set_vertex_data). Keeps the sorted
 * order, radix tree, leaf collapse and node set; recomputes triangle records, boxes and node
 * records (skips Morton codes, sort and emit). Frames are exact as after a rebuild; traversal cost
 * grows as the geometry drifts from the topology. BM_ERROR_INVALID_PARAMETER when the mesh set or
 * a triangle count changed. stats as bm_scene_build (build_ms = the refit's device time). */
int32_t bm_scene_refit(bm_scene* s, bm_build_stats* stats);
/* Reference-mode scenes: out[0] leaves holding faces, out[1] face references stored, out[2] faces
 * dropped by the 256 cap, out[3] largest leaf (before the cap). Synchronous. */
int32_t bm_scene_kd_stats(bm_scene* s, uint64_t out[4]);
/* Reference-mode scenes, for tests: the last build's kd-tree as the march reads it. With L = out[0] of
 * bm_scene_kd_stats and M = *num_pairs (the (leaf, face) pairs, = the sum of leaf_count):
 *   leaf_key[L]    31-bit root-to-leaf paths (depth 0 in the highest of the leaf-depth bits, right = 1),
 *                  ascending
 *   leaf_start[L], leaf_count[L]  leaf i holds faces[leaf_start[i] .. + leaf_count[i]); the count is the
 *                  one before the 256 cap (the march tests the first 256)
 *   faces[M]       global triangle ids, ascending within a leaf
 *   lch, rch, first, last [L - 1]  the radix tree over the leaf keys (root = node 0): a child is an
 *                  internal node's index, or a leaf's index with bit 31 (0x80000000) set; node i covers
 *                  leaves first[i] .. last[i]. Nothing is written for L < 2.
 * Any pointer may be NULL (call once with num_pairs alone to size faces). Synchronous; launches nothing.
 * BM_ERROR_NOT_BUILT before a build, BM_ERROR_INVALID_PARAMETER on a scene of another mode. */
int32_t bm_scene_kd_export(bm_scene* s, uint64_t* num_pairs, uint32_t* leaf_key, uint32_t* leaf_start,
                           uint32_t* leaf_count, uint32_t* faces, uint32_t* lch, uint32_t* rch, uint32_t* first,
                           uint32_t* last);
/* Hashed-grid scenes: out[0] (cell, face) pairs, out[1] non-empty buckets, out[2] largest bucket,
 * out[3] faces beyond the 256 cap. Synchronous. (Hash.cu:82-89, BuildTree.cuh:21) */
int32_t bm_scene_grid_stats(bm_scene* s, uint64_t out[4]);
/* Hashed-grid scenes: bucket b holds faces[bucket_start[b] .. bucket_end[b]) (65,536 buckets; faces
 * = global triangle ids, out[0] of bm_scene_grid_stats entries). Any pointer may be NULL. */
int32_t bm_scene_grid_export(bm_scene* s, uint32_t* bucket_start, uint32_t* bucket_end, uint32_t* faces);
void bm_scene_destroy(bm_scene* s);

/* ---- ray queries: closest hit and any hit over a caller's batch of rays ---------------------
 * The reference traces only its camera's rays; this is the same BVH4 traversal (ray quads) over
 * n rays the caller wrote to device memory: ambient occlusion, bounces, picking, visibility and
 * line-of-sight probes, anything that computes its origins and directions on the device.
 * rays_dev and out_dev are device pointers on the context's device, 16-byte aligned. The work is
 * enqueued on the context stream (after earlier builds and refits, before later ones) and the call
 * returns without waiting; bm_sync waits. On a multi-device context the query runs on the root
 * device alone. dir need not be normalised: t is in units of dir.
 * BM_RAYS_CLOSEST: out_dev is bm_hit[n]. The closest triangle with 0 < t <= tmax (tmax = +inf:
 *   unbounded), equal t resolved to the lowest global triangle id; u, v are its Möller-Trumbore
 *   barycentrics. A miss writes t = +inf, u = v = 0, tri_id = BM_NO_TRIANGLE.
 * BM_RAYS_ANY_HIT: out_dev is uint8_t[n], 1 when any triangle has 0 < t < 1 along the segment
 *   origin -> origin + dir (the shadow rule of bm_camera_trace_shadow), else 0. tmax is ignored in
 *   this mode.
 * Invalid rays (a non-finite origin or direction component; closest mode: tmax NaN or <= 0) are not
 * traced: they get the miss record, or 0.
 * flags: 0, or the filter bits below (BM_RAYS_CULL_*, BM_RAYS_PAD_*); with flags = 0 pad is ignored.
 *   Rays are traced in the order given, 16 consecutive rays per wave: neighbours that start and
 *   point alike share their node fetches.
 * BM_ERROR_INVALID_PARAMETER: a null handle, a null pointer with n > 0, a misaligned pointer, an
 * unknown mode or flag bit, both cull flags or more than one BM_RAYS_PAD_* flag, a scene of a
 * reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has no current build. n = 0
 * succeeds without a launch; over an empty built scene every ray misses.
 *
 * Filters (flags of bm_scene_trace_rays, bm_scene_trace_rays_multi and their counting forms; in the
 * multi-hit calls they combine freely with BM_MULTI_COUNT_ALL). The set of triangles a ray accepts
 * is the unfiltered one (0 < t <= tmax, any hit: 0 < t < 1, multi-hit: H_i below) intersected with
 * the filter: a pure function of the call's flags, the ray's pad word, the candidate's global
 * triangle id g, its det and t of the triangle function (stated at the multi-hit queries below) and
 * the mask of the scene entry that owns g.
 *   BM_RAYS_CULL_BACK      accept only det > 0. det = dot(e1, cross(d, e2)) is the triangle function's
 *                          own; det > 0 <=> the ray runs against cross(e1, e2), the BM_ATTR_GEOM_NORMAL
 *                          direction: a front-facing hit.
 *   BM_RAYS_CULL_FRONT     accept only det < 0.
 *   BM_RAYS_PAD_SKIP_TRI   pad is a global triangle id that is never accepted (the triangle a
 *                          secondary ray starts on: the exact cure for self-intersection).
 *                          BM_NO_TRIANGLE, or an id >= the built triangle count, skips nothing.
 *   BM_RAYS_PAD_TMIN       pad holds the bits of a float tmin: accept t > tmin in place of t > 0 (any
 *                          hit: tmin < t < 1). tmin must be finite and >= 0; a NaN, negative or
 *                          infinite tmin makes the ray invalid (the miss record or 0, not traced).
 *                          tmin >= tmax is valid and misses.
 *   BM_RAYS_PAD_MASK       pad is a 32-bit ray mask: accept when (entry_mask[m(g)] & pad) != 0, m(g)
 *                          the scene entry that owns g (bm_scene_set_entry_mask). pad = 0 is valid and
 *                          misses everything.
 * A triangle the triangle function accepts never has det == 0 (its u is then +-inf or NaN and its t
 *   NaN), so front and back partition the unfiltered accepted set. Instances: facing is that of the
 *   world-space triangle, so a mirroring matrix flips it exactly as it flips BM_ATTR_GEOM_NORMAL.
 * Equal t resolves to the lowest id among the triangles the filter accepts: with a mesh added twice
 *   on one spot, skipping g returns its twin at the same t. A rejected triangle never tightens the
 *   traversal's bound (the closest t, the multi-hit list and its last t); the box test is the
 *   unfiltered one, conservative for any tmin >= 0. Results equal a brute force over all triangles
 *   bit for bit.
 * Counters of filtered calls: out[0] and out[1] as without a filter (node records fetched, a leaf's
 *   triangle count per leaf reached; any hit: the tests up to the first accepted occluder), out[2]
 *   counts hits after the filter. A filter that can reject nothing (BM_RAYS_PAD_SKIP_TRI with pad =
 *   BM_NO_TRIANGLE, BM_RAYS_PAD_TMIN with pad = 0.0f, BM_RAYS_PAD_MASK with pad = 0xFFFFFFFF over
 *   default masks) gives the results and all counters of flags = 0, bit for bit.
 * BM_RAYS_CULL_BACK | BM_RAYS_CULL_FRONT together, or more than one BM_RAYS_PAD_* flag (one call
 *   gives pad one meaning), is BM_ERROR_INVALID_PARAMETER. */
#define BM_RAYS_CULL_BACK 0x10u
#define BM_RAYS_CULL_FRONT 0x20u
#define BM_RAYS_PAD_SKIP_TRI 0x40u
#define BM_RAYS_PAD_TMIN 0x80u
#define BM_RAYS_PAD_MASK 0x100u
typedef struct bm_ray {
    float origin[3];
    float tmax;
    float dir[3];
    uint32_t pad;
} bm_ray; /* 32 B */
typedef struct bm_hit {
    float t, u, v;
    uint32_t tri_id;
} bm_hit; /* 16 B */
#define BM_RAYS_CLOSEST 0u
#define BM_RAYS_ANY_HIT 1u
int32_t bm_scene_trace_rays(bm_scene* s, const bm_ray* rays_dev, uint32_t n, uint32_t mode,
                            uint32_t flags, void* out_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle tests,
 * out[2] hits (closest) or occluded rays (any hit); invalid rays count nothing. Results are written
 * exactly as bm_scene_trace_rays writes them. Synchronous. */
int32_t bm_scene_trace_rays_counters(bm_scene* s, const bm_ray* rays_dev, uint32_t n, uint32_t mode,
                                     uint32_t flags, void* out_dev, uint64_t out[3]);

/* Entry masks: one 32-bit visibility mask per scene entry (index: the entry index of the instance
 * section below, plain and instance entries alike), read by BM_RAYS_PAD_MASK queries only — camera
 * traces, shadow traces, point queries and unflagged ray queries never read them. Every new entry
 * has 0xFFFFFFFF. The mask belongs to its entry: it survives bm_scene_build and bm_scene_refit, moves
 * down with its entry when an earlier one is removed, and dies with it. Setting a mask launches
 * nothing and does not unbuild the scene; it applies to queries enqueued after the call (earlier
 * ones keep the old value, by stream order). The owner of a triangle is found from the entries'
 * triangle counts of the last build.
 * BM_ERROR_INVALID_PARAMETER: a null handle, an index past the entries, a null mask_out. */
int32_t bm_scene_set_entry_mask(bm_scene* s, uint32_t index, uint32_t mask);
int32_t bm_scene_get_entry_mask(const bm_scene* s, uint32_t index, uint32_t* mask_out);

/* ---- multi-hit ray queries: the k nearest hits of each ray, and hit counts --------------------
 * What lies behind the first surface: the first k layers along a ray in order (transparency, X-ray
 * views, depth peeling), entry/exit pairs (thickness, attenuation) and the number of crossings (its
 * parity: inside or outside). One traversal per ray; no origin is moved, so coincident surfaces
 * (a mesh added twice, two instances on one spot) are neither dropped nor counted twice.
 * rays_dev and hits_dev are device pointers on the context's device, 16-byte aligned, counts_dev
 * 4-byte aligned. The work is enqueued on the context stream and the call returns without waiting;
 * bm_sync waits. On a multi-device context the query runs on the root device alone. dir need not be
 * normalised: t is in units of dir.
 * For ray i with origin o, direction d and tmax, H_i is the set of ALL triangles g of the scene that
 *   the triangle function below accepts with 0 < t_g < FLT_MAX and t_g <= tmax (tmax = +inf:
 *   unbounded), ordered by (t_g, g) ascending: equal t resolves to the lower global triangle id.
 * The triangle function of o, d and the triangle's v0, e1 = v1 - v0, e2 = v2 - v0 (each one float32
 *   subtraction per component), in float32, one rounding per operation in the order written, never
 *   contracted; dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z; cross(a,b) = (a.y*b.z - b.y*a.z,
 *   a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y); a comparison with NaN is false; the division is correctly
 *   rounded; there is no determinant epsilon:
 *     p = cross(d,e2)     det = dot(e1,p)     inv = 1 / det
 *     tv = o - v0         u = dot(tv,p) * inv
 *     u < 0 || u > 1      -> rejected
 *     q = cross(tv,e1)    v = dot(d,q) * inv
 *     v < 0 || v + u > 1  -> rejected
 *     t = dot(e2,q) * inv
 *   A NaN t is never accepted (0 < t is false). This is the closest-hit query's own test: record 0
 *   below equals what BM_RAYS_CLOSEST writes for the same ray, bit for bit.
 * hits_dev is bm_hit[n * k]. hits_dev[i*k + j] for j < min(k, |H_i|) is the j-th element of H_i as
 *   {t, u, v, tri_id}; the remaining records of the ray's k are the miss record (t = +inf, u = v = 0,
 *   tri_id = BM_NO_TRIANGLE). The n * k records feed bm_scene_hit_attributes as they are.
 * Without BM_MULTI_COUNT_ALL: k is 1..BM_MULTI_MAX_HITS; counts_dev may be NULL, otherwise
 *   counts_dev[i] = min(k, |H_i|). The traversal prunes by the k-th t once the list is full.
 * With BM_MULTI_COUNT_ALL: counts_dev is required and counts_dev[i] = |H_i|, every crossing within
 *   tmax; the traversal is pruned by tmax alone. k is 0..BM_MULTI_MAX_HITS; with k = 0 hits_dev may
 *   be NULL and nothing is written to it (a pure crossing count).
 * Invalid rays (a non-finite origin or direction component, tmax NaN or <= 0) are not traced: k miss
 *   records, count 0. Over an empty built scene every ray misses.
 * Rays are traced in the order given, 16 consecutive rays per wave, as by bm_scene_trace_rays. The
 *   range note at bm_camera_trace (origins within BM_ENVELOPE_EXTENTS) applies unchanged: the box
 *   test is the same.
 * BM_ERROR_INVALID_PARAMETER: a null handle; with n > 0 a null rays_dev, a null hits_dev while k > 0,
 * a null counts_dev with BM_MULTI_COUNT_ALL; a misaligned pointer; k out of range; an unknown flag
 * bit; a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has no
 * current build. n = 0 succeeds without a launch. */
#define BM_MULTI_MAX_HITS 16u
#define BM_MULTI_COUNT_ALL 1u /* flags; the filter bits BM_RAYS_CULL_* / BM_RAYS_PAD_* above combine with it: H_i
                               * is then the filtered set, and an invalid tmin (BM_RAYS_PAD_TMIN) an invalid ray */
int32_t bm_scene_trace_rays_multi(bm_scene* s, const bm_ray* rays_dev, uint32_t n, uint32_t k,
                                  uint32_t flags, bm_hit* hits_dev, uint32_t* counts_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle tests (a
 * leaf's triangle count per leaf reached), out[2] hit records written (the sum of min(k, |H_i|)) or,
 * with BM_MULTI_COUNT_ALL, the sum of |H_i|; invalid rays count nothing. With k = 1 and no flag,
 * out[0] and out[1] are those of bm_scene_trace_rays_counters in closest mode. Results are written
 * exactly as bm_scene_trace_rays_multi writes them. Synchronous. */
int32_t bm_scene_trace_rays_multi_counters(bm_scene* s, const bm_ray* rays_dev, uint32_t n, uint32_t k,
                                           uint32_t flags, bm_hit* hits_dev, uint32_t* counts_dev,
                                           uint64_t out[3]);

/* ---- closest-point queries: the nearest triangle to each point of a batch ----------------------
 * For point i: which triangle of the scene is nearest, how far, and where on it — unsigned distance
 * fields, point-cloud-to-mesh losses, proximity tests, snapping and projecting points onto a surface.
 * A distance-ordered traversal of the same BVH4, pruned by box distance.
 * points_dev and out_dev are device pointers on the context's device, 16-byte aligned. The work is
 * enqueued on the context stream and the call returns without waiting; bm_sync waits. On a
 * multi-device context the query runs on the root device alone.
 * Result i is a bm_hit: t the distance sqrtf(dd), u and v the barycentrics of the closest point in
 *   the hit-attribute convention (the point is v0*(1-(u+v)) + v1*u + v2*v), tri_id the global id. It
 *   feeds bm_scene_hit_attributes as it is: BM_VERTEX_DATA_POSITION is then the closest point,
 *   BM_VERTEX_DATA_NORMAL the normal there, BM_ATTR_MESH_FACE the owner (instanced scenes included:
 *   their triangles are in world space).
 * The winner is the lexicographic minimum of (dd_g, g) over ALL triangles g of the scene with
 *   dd_g <= rmax*rmax (one float32 multiply; rmax = +inf: unbounded): equal dd resolves to the lowest
 *   id. Without such a triangle, over an empty scene and for an invalid point (a non-finite component
 *   of p; rmax NaN or <= 0) the record is the ray query's miss: t = +inf, u = v = 0, tri_id =
 *   BM_NO_TRIANGLE.
 * dd_g is this function of p and the triangle's v0, e1 = v1 - v0, e2 = v2 - v0 (each one float32
 *   subtraction per component), in float32, one rounding per operation in the order written, never
 *   contracted; dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z; a comparison with NaN is false:
 *     ap = p - v0
 *     d1 = dot(e1,ap)   d2 = dot(e2,ap)
 *     a11 = dot(e1,e1)  a12 = dot(e1,e2)  a22 = dot(e2,e2)
 *     d3 = d1 - a11     d4 = d2 - a12     d5 = d1 - a12     d6 = d2 - a22
 *     1. d1 <= 0 && d2 <= 0                          -> u = 0, v = 0
 *     2. d3 >= 0 && d4 <= d3                         -> u = 1, v = 0
 *     3. vc = d1*d4 - d3*d2;  vc <= 0 && d1 >= 0 && d3 <= 0
 *                                                    -> u = d1 / (d1 - d3), v = 0
 *     4. d6 >= 0 && d5 <= d6                         -> u = 0, v = 1
 *     5. vb = d5*d2 - d1*d6;  vb <= 0 && d2 >= 0 && d6 <= 0
 *                                                    -> u = 0, v = d2 / (d2 - d6)
 *     6. va = d3*d6 - d5*d4;  s = d4 - d3; r = d5 - d6;  va <= 0 && s >= 0 && r >= 0
 *                                                    -> w = s / (s + r);  u = 1 - w, v = w
 *     7. otherwise   den = 1 / ((va + vb) + vc);        u = vb*den, v = vc*den
 *     q = ap - (e1*u + e2*v)   per component: ap.x - (e1.x*u + e2.x*v)
 *     dd = dot(q,q)
 *   The first matching region wins; divisions and sqrtf are correctly rounded. A triangle whose dd is
 *   NaN is never a candidate (dd < best is false). A zero-area triangle has va = vb = vc = 0 up to
 *   rounding: it counts through its vertex regions and through an edge region whose division is not
 *   0/0, and where rounding sends it to region 7 with a zero sum it does not count at all — as rays do
 *   not hit degenerate triangles either.
 * flags: none defined yet, pass 0. Points are taken in the order given, 16 consecutive points per wave.
 * BM_ERROR_INVALID_PARAMETER: a null handle, a null pointer with n > 0, a misaligned pointer, a flag
 * bit, a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has no current
 * build. n = 0 succeeds without a launch. */
typedef struct bm_point {
    float p[3];
    float rmax;
} bm_point; /* 16 B */
int32_t bm_scene_closest_points(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t flags,
                                bm_hit* out_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle evaluations,
 * out[2] points with a result, out[3] the largest number of stack entries any query held at once (above
 * 24 the traversal used the global overflow area); invalid points count nothing. Results are written
 * exactly as bm_scene_closest_points writes them. Synchronous. */
int32_t bm_scene_closest_points_counters(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t flags,
                                         bm_hit* out_dev, uint64_t out[4]);

/* ---- multi-result point queries: the k nearest triangles to each point, and how many lie within r
 * The point side's counterpart of bm_scene_trace_rays_multi. For point i: all triangles within rmax,
 * each with its closest point (the contact set of a sphere collider: with bm_scene_hit_attributes the
 * contact point and normal per triangle, the penetration depth rmax - t); the k nearest triangles
 * (robust normals and signs near edges and creases, where the single nearest triangle is arbitrary
 * among several at equal distance; blended distance fields; point-cloud-to-mesh losses with more than
 * one candidate); and the number of triangles within rmax (a density or "is anything near" probe
 * that writes no records, or the size of a second pass). One traversal per point.
 * points_dev and hits_dev are device pointers on the context's device, 16-byte aligned, counts_dev
 * 4-byte aligned. The work is enqueued on the context stream and the call returns without waiting;
 * bm_sync waits. On a multi-device context the query runs on the root device alone.
 * For point i with p and rmax, N_i is the set of ALL triangles g of the scene whose dd_g is not NaN
 *   and dd_g <= rmax*rmax (one float32 multiply; rmax = +inf: unbounded), ordered by (dd_g, g)
 *   ascending: equal distance resolves to the lower global triangle id. dd_g, u and v are the
 *   closest-point section's function of p and the triangle, as stated there.
 * hits_dev is bm_hit[n * k]. hits_dev[i*k + j] for j < min(k, |N_i|) is the j-th element of N_i as
 *   {t = sqrtf(dd), u, v, tri_id} in bm_scene_closest_points' convention; the remaining records of the
 *   point's k are the miss record (t = +inf, u = v = 0, tri_id = BM_NO_TRIANGLE). The n * k records
 *   feed bm_scene_hit_attributes as they are.
 * Without BM_MULTI_COUNT_ALL: k is 1..BM_MULTI_MAX_HITS; counts_dev may be NULL, otherwise
 *   counts_dev[i] = min(k, |N_i|). With k = 1, record 0 equals what bm_scene_closest_points writes
 *   for the same point, bit for bit.
 * With BM_MULTI_COUNT_ALL: counts_dev is required and counts_dev[i] = |N_i|, every triangle within
 *   rmax. k is 0..BM_MULTI_MAX_HITS; with k = 0 hits_dev may be NULL and nothing is written to it (a
 *   pure count).
 * Invalid points (a non-finite component of p; rmax NaN or <= 0) are not looked up: k miss records,
 *   count 0. Over an empty built scene every point misses.
 * Points are taken in the order given, 16 consecutive points per wave, as by bm_scene_closest_points.
 * BM_ERROR_INVALID_PARAMETER: a null handle; with n > 0 a null points_dev, a null hits_dev while
 * k > 0, a null counts_dev with BM_MULTI_COUNT_ALL; a misaligned pointer; k out of range; an unknown
 * flag bit; a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has no
 * current build. n = 0 succeeds without a launch. */
int32_t bm_scene_closest_points_multi(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t k,
                                      uint32_t flags, bm_hit* hits_dev, uint32_t* counts_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle evaluations (a
 * leaf's triangle count per leaf reached), out[2] records written (the sum of min(k, |N_i|)) or, with
 * BM_MULTI_COUNT_ALL, the sum of |N_i|, out[3] the largest number of stack entries any query held at
 * once; invalid points count nothing. With k = 1 and no flag, out[0] and out[1] are those of
 * bm_scene_closest_points_counters. Results are written exactly as bm_scene_closest_points_multi
 * writes them. Synchronous. */
int32_t bm_scene_closest_points_multi_counters(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t k,
                                               uint32_t flags, bm_hit* hits_dev, uint32_t* counts_dev,
                                               uint64_t out[4]);

/* ---- sphere-cast queries: the first contact of a swept sphere per ray ---------------------------
 * How far can a sphere of radius r travel along a direction before it touches the mesh, and where does it
 * touch: camera collision, character and projectile controllers, thick line of sight, clearance along a
 * tool path, continuous collision of particles. A few ordinary rays miss edges and vertices between them
 * and tunnel through thin features; a radius query answers only the stationary case.
 * sweeps_dev and out_dev are device pointers on the context's device, 16-byte aligned. The work is
 * enqueued on the context stream and the call returns without waiting; bm_sync waits. On a multi-device
 * context the query runs on the root device alone.
 * A sweep is a bm_ray whose pad word is the radius. The sphere's centre moves as c(t) = origin + t*dir for
 *   0 <= t <= tmax; dir need not be normalised (t is in units of dir), tmax = +inf means unbounded.
 * BM_SWEEP_CLOSEST: out_dev is bm_hit[n]. The result is the lexicographic minimum of (t_g, g) over ALL
 *   triangles g of the scene for which the triangle function below returns a t_g with 0 <= t_g <= tmax
 *   and t_g <= FLT_MAX: equal t resolves to the lowest id. u and v are the barycentrics of the contact
 *   point on the triangle in the hit-attribute convention (the point is v0*(1-(u+v)) + v1*u + v2*v). A
 *   sphere that already touches or overlaps triangle g at the start has t_g = 0 with the (u, v) of the
 *   closest-point function at the origin. Without such a triangle, over an empty scene and for an invalid
 *   sweep the record is the ray query's miss: t = +inf, u = v = 0, tri_id = BM_NO_TRIANGLE. The record
 *   feeds bm_scene_hit_attributes as it is: BM_VERTEX_DATA_POSITION is then the contact point, and
 *   c(t) - contact is the sphere's contact normal.
 * BM_SWEEP_ANY: out_dev is uint8_t[n]: 1 when any triangle has such a t_g, else 0; the traversal stops at
 *   the first one. tmax is honoured here (unlike BM_RAYS_ANY_HIT, whose segment is 0 < s < 1 whatever
 *   tmax says).
 * Invalid sweeps (a non-finite origin or direction component; an all-zero direction; tmax NaN or negative
 *   — tmax = 0 is valid and asks only about the start; a radius that is NaN, infinite or <= 0) are not
 *   traversed: the miss record, or 0.
 * The triangle function of o = origin, d = dir, r = radius, tl = min(tmax, FLT_MAX) and the triangle's
 *   v0, e1 = v1 - v0, e2 = v2 - v0 (each one float32 subtraction per component), in float32, one rounding
 *   per operation in the order written, never contracted; dot and cross as stated at the multi-hit
 *   queries; divisions and sqrtf correctly rounded; a comparison with NaN is false:
 *     start:  dd0, u0, v0 = the closest-point section's function of o;   rr = r*r
 *             dd0 <= rr  ->  t = 0, u = u0, v = v0
 *     ap = o - v0        dd = dot(d,d)
 *     1. face:   n = cross(e1,e2)   nn = dot(n,n)   h = dot(n,ap)   nd = dot(n,d)   ln = sqrtf(nn)
 *                hs = |h|   nds = h >= 0 ? nd : -nd      t = (hs - r*ln) / (-nds)
 *                w = ap + d*t   per component: ap.x + d.x*t
 *                u = dot(n, cross(w,e2)) / nn      v = dot(n, cross(e1,w)) / nn
 *                accepted: nds < 0 && u >= 0 && v >= 0 && u + v <= 1 && t >= 0 && t <= tl
 *     edge(m, E, md, mm):  EE = dot(E,E)   Ed = dot(E,d)   Em = dot(E,m)
 *                qa = EE*dd - Ed*Ed    qb = EE*md - Ed*Em    qc = EE*(mm - rr) - Em*Em
 *                disc = qb*qb - qa*qc    t = (-qb - sqrtf(disc)) / qa    s = (Em + t*Ed) / EE
 *                accepted: disc >= 0 && qa > 0 && s >= 0 && s <= 1 && t >= 0 && t <= tl
 *     vertex(md, mm):      disc = md*md - dd*(mm - rr)    t = (-md - sqrtf(disc)) / dd
 *                accepted: disc >= 0 && dd > 0 && t >= 0 && t <= tl
 *     md0 = dot(ap,d)  mm0 = dot(ap,ap)   m1 = ap - e1  md1 = dot(m1,d)  mm1 = dot(m1,m1)
 *     m2 = ap - e2  md2 = dot(m2,d)  mm2 = dot(m2,m2)
 *     2. edge(ap, e1, md0, mm0)       -> u = s, v = 0
 *     3. edge(ap, e2, md0, mm0)       -> u = 0, v = s
 *     4. edge(m1, e2 - e1, md1, mm1)  -> u = 1 - s, v = s
 *     5. vertex(md0, mm0) -> u = 0, v = 0    6. vertex(md1, mm1) -> u = 1, v = 0
 *     7. vertex(md2, mm2) -> u = 0, v = 1
 *   Without a start, t_g is the smallest t of the accepted candidates, the earlier one in this list on
 *   equal t; with none accepted the triangle has no t_g. A NaN is never accepted.
 * Resolution: the roots cancel in float32 when the origin is far away compared with r (mm - rr against
 *   mm, and the discriminant's two products). With S the largest |origin - vertex| involved, the centre
 *   at the reported t lies within about 2^-10 * S of distance r from the triangle, and a radius below
 *   about 2^-11 * S is not resolved: such a sphere is swept as if its radius were anything up to that.
 *   The traversal's pruning margin is sized from the same figure, so what it returns is still the
 *   function's minimum over all triangles, bit for bit. Origins within BM_ENVELOPE_EXTENTS of the scene,
 *   as at bm_camera_trace.
 * flags: none defined yet, pass 0 (the pad word is taken: the ray query's filters do not apply). Sweeps are
 * taken in the order given, 16 consecutive sweeps per wave.
 * BM_ERROR_INVALID_PARAMETER: a null handle, a null pointer with n > 0, a misaligned pointer, an unknown
 * mode or any flag bit, a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene
 * has no current build. n = 0 succeeds without a launch. */
typedef struct bm_sweep {
    float origin[3];
    float tmax;
    float dir[3];
    float radius;
} bm_sweep; /* 32 B, bm_ray's layout with pad = radius */
#define BM_SWEEP_CLOSEST 0u
#define BM_SWEEP_ANY 1u
int32_t bm_scene_sweep_spheres(bm_scene* s, const bm_sweep* sweeps_dev, uint32_t n, uint32_t mode,
                               uint32_t flags, void* out_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle evaluations,
 * out[2] sweeps with a result (BM_SWEEP_ANY: sweeps that touch), out[3] the largest number of stack
 * entries any sweep held at once (above 24 the traversal used the global overflow area); invalid sweeps
 * count nothing. Results are written exactly as bm_scene_sweep_spheres writes them. Synchronous. */
int32_t bm_scene_sweep_spheres_counters(bm_scene* s, const bm_sweep* sweeps_dev, uint32_t n, uint32_t mode,
                                        uint32_t flags, void* out_dev, uint64_t out[4]);

/* ---- signed-distance and occupancy queries: inside or outside, for each point of a batch --------
 * The sign the closest-point section leaves out. For point i: is it inside the scene's surface, and what
 * is its signed distance — SDF grids for collision and learning, inside from outside after a
 * voxelisation, the penetration depth of a sphere collider whose centre has gone through the surface, the
 * sign at the end of a simulate / upload / normals / refit / query loop. One call and one launch instead
 * of a ray batch, a crossing count, its parity and a second closest-point launch merged by hand.
 * points_dev and out_dev are device pointers on the context's device, 16-byte aligned; votes_dev needs no
 * alignment. The work is enqueued on the context stream and the call returns without waiting; bm_sync
 * waits. On a multi-device context the query runs on the root device alone.
 * Inside: the sign is crossing parity along fixed sample directions, not pseudonormals or winding
 *   numbers: it asks nothing of the index topology (unshared OBJ ingest, a mesh added twice and
 *   instanced scenes are triangle soups) and is a function of the triangle set alone. For sample
 *   direction D_j the crossing count C_j(p) is the number of ALL triangles of the scene that the
 *   multi-hit section's triangle function accepts for the ray (origin = p, dir = D_j, tmax = +inf):
 *   0 < t < FLT_MAX, no filter — bm_scene_trace_rays_multi's count with k = 0 and BM_MULTI_COUNT_ALL,
 *   exactly. The vote is v_j = C_j & 1. Without BM_SIGNED_VOTE3, inside = v_0; with it,
 *   inside = (v_0 + v_1 + v_2 >= 2).
 *   D0 = (a, b, c), D1 = (-b, c, a), D2 = (c, -a, b) with the float32 constants a = BM_SIGNED_DA,
 *   b = BM_SIGNED_DB, c = BM_SIGNED_DC below (0.80901694, 0.309017, 0.2317616). They have no zero
 *   component and no small-integer ratios, so grid-aligned points against axis-aligned or 45-degree
 *   geometry do not send rays through edges: the triangle function accepts u = 0, v = 0 and u + v = 1,
 *   so a ray through an edge shared by two triangles counts both, and the directions (1,0,0) and (1,1,1)
 *   get hundreds of the points of a 1/8 grid around a cube or an octahedron wrong where these get none.
 *   A closed mesh that is added twice flips the parity back: every point is then outside.
 * votes_dev may be NULL; otherwise it is uint8_t[n] and votes_dev[i] is the sum of the votes taken,
 *   0..1 or with BM_SIGNED_VOTE3 0..3. With BM_SIGNED_VOTE3 a value of 1 or 2 tells the caller that the
 *   mesh is open or that a ray grazed it there.
 * BM_SIGNED_DISTANCE: out_dev is bm_hit[n]. u, v, tri_id and |t| are what bm_scene_closest_points writes
 *   for the same point record, bit for bit (the same dd function, the same (dd, id) minimum, rmax
 *   honoured); the sign bit of t is set when the point is inside, so a point on the surface gives +0 or
 *   -0. With no triangle within rmax the record is the miss record with t = -inf inside and +inf
 *   outside: a narrow-band SDF keeps its sign outside the band. The record feeds
 *   bm_scene_hit_attributes as it is (the id decides a miss there, not t).
 * BM_SIGNED_OCCUPANCY: out_dev is uint8_t[n], 1 inside and 0 outside. No nearest traversal; rmax is not
 *   read.
 * Invalid points: a non-finite component of p; in distance mode also rmax NaN or <= 0. An invalid point
 *   gives the +inf miss record, or 0, and vote 0, and is not traversed. Over an empty built scene every
 *   point is outside.
 * Range: the parity rays go through the ray query's box test, so the BM_ENVELOPE_EXTENTS note of
 *   bm_camera_trace applies to them: points within that many scene extents of the scene.
 * Points are taken in the order given, 16 consecutive points per wave, as by bm_scene_closest_points.
 * BM_ERROR_INVALID_PARAMETER: a null handle, a null points_dev or out_dev with n > 0, a misaligned
 * points_dev or out_dev, an unknown mode or flag bit, a scene of a reference-mode, BVH2 or BVH8 context.
 * BM_ERROR_NOT_BUILT: the scene has no current build. n = 0 succeeds without a launch. */
#define BM_SIGNED_DISTANCE 0u /* mode */
#define BM_SIGNED_OCCUPANCY 1u
#define BM_SIGNED_VOTE3 1u /* flag */
#define BM_SIGNED_DA 0x1.9e3778p-1f
#define BM_SIGNED_DB 0x1.3c6ef4p-2f
#define BM_SIGNED_DC 0x1.daa5d4p-3f
int32_t bm_scene_signed_distances(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t mode,
                                  uint32_t flags, void* out_dev, uint8_t* votes_dev);
/* The counting build of the same query: out[0] BVH node records fetched by the nearest phase, out[1] its
 * triangle evaluations (both as bm_scene_closest_points_counters counts them; 0 in occupancy mode), out[2]
 * node records fetched by the parity phase, out[3] the parity phase's triangle tests (a leaf's triangle
 * count per leaf reached), both summed over the directions taken; invalid points count nothing. Results
 * are written exactly as bm_scene_signed_distances writes them. Synchronous. */
int32_t bm_scene_signed_distances_counters(bm_scene* s, const bm_point* points_dev, uint32_t n, uint32_t mode,
                                           uint32_t flags, void* out_dev, uint8_t* votes_dev, uint64_t out[4]);

/* ---- box overlap queries: the triangles that intersect each box of a batch ---------------------
 * The third family beside rays and points: volumes. For axis-aligned box i: which triangles of the
 * scene touch it — voxelising a mesh into an occupancy grid, selecting a region, the broad phase of
 * box colliders and triggers, binning triangles into cells, bricks or clusters, clipping work to a
 * region of interest. An unordered traversal of the same BVH4 that follows every child box the query
 * box meets.
 * boxes_dev is a device pointer on the context's device, 16-byte aligned; out_dev, offsets_dev and
 * ids_dev are 4-byte aligned (the byte plane of BM_BOXES_ANY: any address). The work is enqueued on the
 * context stream and the call returns without waiting; bm_sync waits. On a multi-device context the
 * query runs on the root device alone.
 * For box i with centre c and half-size h, O_i is the set of ALL triangles g of the scene that
 *   tri_box(c, h, tv) accepts, tv being the triangle as the build's 48-byte record holds it: v0, and
 *   v1 = v0 + e1, v2 = v0 + e2 with e1, e2 the record's edges, one float32 addition per component.
 *   (The record's edges are the mesh's v1 - v0 and v2 - v0 in float32, so v1 and v2 differ from the
 *   mesh's own v1 and v2 only where that subtraction was inexact.) The test is inclusive: a triangle
 *   touching a face of the box is in O_i.
 * tri_box is the reference's triBoxOverlap, the test its kd-tree and hashed grid sort triangles by, in
 *   float32, one rounding per operation in the order written, never contracted; a comparison with NaN
 *   is false. With x, y, z the components 0, 1, 2:
 *     w0 = v0 - c   w1 = v1 - c   w2 = v2 - c            (per component)
 *     f0 = w1 - w0  f1 = w2 - w1  f2 = w0 - w2           (per component)
 *     sep(pa, pb, rad): with mn, mx = (pa < pb) ? (pa, pb) : (pb, pa):   mn > rad || mx < -rad
 *     X(f, a, b):  sep(f.z*a.y - f.y*a.z,   f.z*b.y - f.y*b.z,   |f.z|*h.y + |f.y|*h.z)
 *     Y(f, a, b):  sep(-f.z*a.x + f.x*a.z, -f.z*b.x + f.x*b.z,  |f.z|*h.x + |f.x|*h.z)
 *     Z(f, a, b):  sep(f.y*b.x - f.x*b.y,   f.y*a.x - f.x*a.y,   |f.y|*h.x + |f.x|*h.y)   (b's value first)
 *     Z0(f, a, b): sep(f.y*a.x - f.x*a.y,   f.y*b.x - f.x*b.y,   |f.y|*h.x + |f.x|*h.y)
 *     the nine cross-axis tests:  X(f0, w0, w2)  Y(f0, w0, w2)  Z(f0, w1, w2)
 *                                 X(f1, w0, w2)  Y(f1, w0, w2)  Z0(f1, w0, w1)
 *                                 X(f2, w0, w1)  Y(f2, w0, w1)  Z(f2, w1, w2)
 *     the AABB test, per axis k:  mn = mx = w0.k; if (w1.k < mn) mn = w1.k; if (w1.k > mx) mx = w1.k;
 *                                 the same with w2.k;   mn > h.k || mx < -h.k
 *     the plane test:  nrm = (f0.y*f1.z - f0.z*f1.y, f0.z*f1.x - f0.x*f1.z, f0.x*f1.y - f0.y*f1.x);
 *                      per axis k: nrm.k > 0 ? (lo.k = -h.k - w0.k, hi.k = h.k - w0.k)
 *                                            : (lo.k = h.k - w0.k, hi.k = -h.k - w0.k);
 *                      passes when !(dot(nrm, lo) > 0) && dot(nrm, hi) >= 0,
 *                      dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   tri_box accepts when none of the nine cross-axis tests and none of the three AABB tests is true and
 *   the plane test passes. (-f.z*a.x is the product of the negated f.z.) A zero-area triangle has a
 *   zero normal and zero radii on the axes of its vanished edges: it is accepted when the remaining
 *   tests do not separate it, so a point-like or segment-like triangle inside a box is in O_i.
 * mode BM_BOXES_COUNT: out_dev is uint32_t[n], out_dev[i] = |O_i|. offsets_dev and ids_dev are ignored.
 * mode BM_BOXES_ANY: out_dev is uint8_t[n], out_dev[i] = 1 when O_i is not empty, else 0. The traversal
 *   of a box ends at the first accepted triangle.
 * mode BM_BOXES_LIST: a CSR (compressed sparse row) fill. offsets_dev is uint32_t[n + 1], ascending:
 *   normally the exclusive prefix sum of a count pass, but any segmentation is allowed (i * stride, say).
 *   The ids of O_i are written to ids_dev[offsets_dev[i] ..], at most offsets_dev[i+1] - offsets_dev[i]
 *   of them; nothing is ever written outside a box's own segment, and the unused tail of a segment is
 *   left untouched. out_dev may be NULL; otherwise it is uint32_t[n] and out_dev[i] = |O_i|, so a caller
 *   whose segments were too short can tell. The order inside a segment is the traversal's: the same for
 *   every call on the same build, on every GPU and grid size (nothing is decided by an atomic), and
 *   otherwise unspecified. When a segment is too short it holds the first ids of that order.
 * Invalid boxes (a non-finite component of c or h; a component of h that is negative or NaN) are not
 *   looked up: count 0, byte 0, no ids. h = 0 is valid (the box is a point). The pad words are ignored.
 *   Over an empty built scene every count and byte is 0.
 * flags: none defined yet, pass 0. Boxes are taken in the order given, 16 consecutive boxes per wave.
 * BM_ERROR_INVALID_PARAMETER: a null handle; with n > 0 a null boxes_dev, a null out_dev unless the mode
 * is BM_BOXES_LIST, a null offsets_dev or ids_dev with BM_BOXES_LIST; a misaligned pointer; an unknown
 * mode or flag bit; a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has
 * no current build. n = 0 succeeds without a launch. */
typedef struct bm_box {
    float center[3];
    uint32_t pad0;
    float half[3];
    uint32_t pad1;
} bm_box; /* 32 B */
#define BM_BOXES_COUNT 0u
#define BM_BOXES_ANY 1u
#define BM_BOXES_LIST 2u
int32_t bm_scene_overlap_boxes(bm_scene* s, const bm_box* boxes_dev, uint32_t n, uint32_t mode, uint32_t flags,
                               void* out_dev, const uint32_t* offsets_dev, uint32_t* ids_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle tests (a leaf's
 * triangle count per leaf reached), out[2] the sum of |O_i| (BM_BOXES_ANY: the number of boxes with a
 * hit), out[3] the largest number of stack entries any box held at once (above 24 the traversal used the
 * global overflow area); invalid boxes count nothing. Results are written exactly as
 * bm_scene_overlap_boxes writes them. Synchronous. */
int32_t bm_scene_overlap_boxes_counters(bm_scene* s, const bm_box* boxes_dev, uint32_t n, uint32_t mode,
                                        uint32_t flags, void* out_dev, const uint32_t* offsets_dev,
                                        uint32_t* ids_dev, uint64_t out[4]);

/* ---- triangle overlap queries: the scene triangles each triangle of a batch intersects ----------
 * The volume family's mesh-against-mesh question: a collider that is a mesh and not a box, a tool swept
 * through a part, the intersection curve a boolean operation starts from, the self-intersections mesh
 * repair looks for. For query triangle i: which triangles of the scene it touches. An unordered
 * traversal of the same BVH4 that follows every child box the query triangle's own bounds meet.
 * tris_dev is a device pointer on the context's device, 16-byte aligned; out_dev, offsets_dev and
 * ids_dev are 4-byte aligned (the byte plane of BM_TRIS_ANY: any address). The work is enqueued on the
 * context stream and the call returns without waiting; bm_sync waits. On a multi-device context the
 * query runs on the root device alone.
 * For query triangle a (vertices a0, a1, a2), O_i is the set of ALL triangles g of the scene that
 *   tri_tri(a, b) accepts, b being g as the build's 48-byte record holds it: b0 = v0, b1 = v0 + e1,
 *   b2 = v0 + e2 with e1, e2 the record's edges, one float32 addition per component (as for
 *   bm_scene_overlap_boxes). The test is inclusive: triangles that touch intersect.
 * tri_tri is a separating-axis test in float32, one rounding per operation in the order written, never
 *   contracted; a comparison with NaN is false. With x, y, z the components 0, 1, 2:
 *     the AABB part, on the raw coordinates, per axis k:
 *       qlo = qhi = a0.k; if (a1.k < qlo) qlo = a1.k; if (a1.k > qhi) qhi = a1.k; the same with a2.k;
 *       blo, bhi likewise from b0.k, b1.k, b2.k;         meets.k:  blo <= qhi && bhi >= qlo
 *     the separating-axis part, on coordinates translated by a0 (so that a scene far from the origin
 *     keeps the test's resolution), per component:
 *       p1 = a1 - a0   p2 = a2 - a0   (p0 = 0)           q0 = b0 - a0   q1 = b1 - a0   q2 = b2 - a0
 *       eA0 = p1   eA1 = p2 - p1   eA2 = 0 - p2          eB0 = q1 - q0  eB1 = q2 - q1  eB2 = q0 - q2
 *       cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)
 *       dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z
 *       nA = cross(eA0, eA1)   nB = cross(eB0, eB1)
 *       sep(d): s1 = dot(d, p1), s2 = dot(d, p2); mnA = mxA = 0; if (s1 < mnA) mnA = s1;
 *               if (s1 > mxA) mxA = s1; the same with s2;
 *               t0 = dot(d, q0), t1 = dot(d, q1), t2 = dot(d, q2); mnB = mxB = t0; if (t1 < mnB) mnB = t1;
 *               if (t1 > mxB) mxB = t1; the same with t2;        mxA < mnB || mxB < mnA
 *       the seventeen axes, in this order: nA; nB; cross(eA_i, eB_j) for i = 0..2 (outer), j = 0..2;
 *       cross(nA, eA_i) for i = 0..2; cross(nB, eB_j) for j = 0..2
 *   tri_tri accepts when meets.k holds on all three axes and sep(d) is false for all seventeen axes.
 *   An axis that vanishes (parallel edges, a zero normal) projects everything to 0 and separates
 *   nothing, so degenerate triangles of either side (point-like, segment-like) are accepted exactly when
 *   the remaining axes do not separate them. The six in-plane axes cross(n, e) are what reject coplanar
 *   triangles that lie apart. The translation makes the test not bit-symmetric: tri_tri(a, b) and
 *   tri_tri(b, a) can differ by roundings at contact.
 * mode BM_TRIS_COUNT: out_dev is uint32_t[n], out_dev[i] = |O_i|. offsets_dev and ids_dev are ignored.
 * mode BM_TRIS_ANY: out_dev is uint8_t[n], out_dev[i] = 1 when O_i is not empty, else 0. The traversal
 *   of a query ends at the first accepted triangle.
 * mode BM_TRIS_LIST: a CSR (compressed sparse row) fill, by BM_BOXES_LIST's rules. offsets_dev is
 *   uint32_t[n + 1], ascending: normally the exclusive prefix sum of a count pass, but any segmentation
 *   is allowed. The ids of O_i are written to ids_dev[offsets_dev[i] ..], at most
 *   offsets_dev[i+1] - offsets_dev[i] of them; nothing is ever written outside a query's own segment,
 *   and the unused tail of a segment is left untouched. out_dev may be NULL; otherwise it is uint32_t[n]
 *   and out_dev[i] = |O_i|. The order inside a segment is the traversal's: the same for every call on
 *   the same build, on every GPU and grid size (nothing is decided by an atomic), and otherwise
 *   unspecified. When a segment is too short it holds the first ids of that order.
 * Invalid query triangles (any non-finite vertex component) are not looked up: count 0, byte 0, no ids.
 *   Degenerate query triangles are valid. Over an empty built scene every count and byte is 0.
 * flags: 0, or BM_TRIS_PAD_SKIP_TRI: pad0 of each record names one triangle id that is never in O_i
 *   (a mesh queried against itself passes each triangle's own id). The filter runs on candidates the
 *   test has accepted, as the ray filters do; NO_TRI (0xFFFFFFFF) or an id past the scene skips nothing.
 *   Without the flag the pad words are ignored; pad1 and pad2 always are.
 * Queries are taken in the order given, 16 consecutive triangles per wave.
 * BM_ERROR_INVALID_PARAMETER: a null handle; with n > 0 a null tris_dev, a null out_dev unless the mode
 * is BM_TRIS_LIST, a null offsets_dev or ids_dev with BM_TRIS_LIST; a misaligned pointer; an unknown
 * mode or flag bit; a scene of a reference-mode, BVH2 or BVH8 context. BM_ERROR_NOT_BUILT: the scene has
 * no current build. n = 0 succeeds without a launch. */
typedef struct bm_tri {
    float v0[3];
    uint32_t pad0;
    float v1[3];
    uint32_t pad1;
    float v2[3];
    uint32_t pad2;
} bm_tri; /* 48 B */
#define BM_TRIS_COUNT 0u
#define BM_TRIS_ANY 1u
#define BM_TRIS_LIST 2u
#define BM_TRIS_PAD_SKIP_TRI 1u /* flag: pad0 is a triangle id that is never in O_i */
int32_t bm_scene_overlap_triangles(bm_scene* s, const bm_tri* tris_dev, uint32_t n, uint32_t mode, uint32_t flags,
                                   void* out_dev, const uint32_t* offsets_dev, uint32_t* ids_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle tests (a leaf's
 * triangle count per leaf reached), out[2] the sum of |O_i| (BM_TRIS_ANY: the number of queries with a
 * hit), out[3] the largest number of stack entries any query held at once (above 24 the traversal used
 * the global overflow area); invalid queries count nothing. Results are written exactly as
 * bm_scene_overlap_triangles writes them. Synchronous. */
int32_t bm_scene_overlap_triangles_counters(bm_scene* s, const bm_tri* tris_dev, uint32_t n, uint32_t mode,
                                            uint32_t flags, void* out_dev, const uint32_t* offsets_dev,
                                            uint32_t* ids_dev, uint64_t out[4]);

/* ---- plane section queries: the triangles each plane of a batch crosses, and their cut segments -----
 * The fourth family: planes. For plane i: where does it cut the scene — the layers of a slicer, cross-sections
 * and contour lines, the cap polygon of a clipping plane, cutting planes of tool paths, the outline a boolean
 * or remeshing step starts from. An unordered traversal of the same BVH4 that follows every child box with a
 * corner on each side of the plane.
 * planes_dev is a device pointer on the context's device, 16-byte aligned, and so is segs_dev; out_dev,
 * offsets_dev and ids_dev are 4-byte aligned (the byte plane of BM_PLANES_ANY: any address). The work is
 * enqueued on the context stream and the call returns without waiting; bm_sync waits. On a multi-device
 * context the query runs on the root device alone.
 * The plane passes through `point` and is perpendicular to `normal`, which need not have unit length.
 * The query is stated on the meshes' own vertices, not on the build's (v0, e1, e2) records: triangle g's
 *   positions x0, x1, x2 are read through its mesh's index triple, in index order, from the mesh's position
 *   slot (an instanced entry: from the scene's world-space copy of the last build or refit). Float32
 *   throughout, one rounding per operation in the order written, never contracted; a comparison with NaN is
 *   false.
 *     For a position x:  d = x - point (per component),  s(x) = (n.x*d.x + n.y*d.y) + n.z*d.z.
 *     x is BELOW when s(x) < 0, otherwise ABOVE: s = +0 or -0 is above, so a vertex on the plane belongs to
 *     the positive side.
 *     Triangle g is CROSSED when at least one of its vertices is below and at least one is above.
 *   C_i is the set of ALL crossed triangles of the scene. Consequences of the rule:
 *     a triangle lying in the plane is not crossed (all three vertices are above);
 *     a triangle that touches the plane from above (a vertex or an edge on it, the rest above) is not crossed;
 *     a triangle that touches the plane from below is crossed, with a segment of length zero (a vertex on
 *     the plane) or the touching edge itself;
 *     both triangles on a mesh edge see the same sides of its two ends, which is what makes every loop close.
 * The segment of a crossed triangle: going x0 -> x1 -> x2 -> x0, exactly one edge runs from above to below
 *   (the down edge) and exactly one from below to above (the up edge). a is the cut of the down edge and b
 *   the cut of the up edge; seen from the triangle's front (the side its counter-clockwise winding faces),
 *   the above side lies to the left of a -> b.
 *   The cut of an edge with below end N and above end P, whichever way the edge runs:
 *     t = s(N) / (s(N) - s(P))         and per component  X = t*P + (N - t*N)
 *   s(N) < 0 <= s(P), so the denominator is never zero and t lies in (0, 1]; t = 1 exactly when P is on the
 *   plane, and X is then P (bit for bit, up to the sign of a zero component).
 *   X depends only on the two positions' bits and the plane: the two triangles on an edge compute identical
 *   bits whatever their vertex indices, unwelded (duplicated) vertices included. On a consistently oriented
 *   closed manifold each crossed edge is one triangle's up edge and the other's down edge, so the multiset of
 *   the b equals the multiset of the a bit for bit, and the segments chain into closed loops by plain
 *   equality of endpoints, with no welding tolerance.
 * mode BM_PLANES_COUNT: out_dev is uint32_t[n], out_dev[i] = |C_i|. offsets_dev, ids_dev, segs_dev ignored.
 * mode BM_PLANES_ANY: out_dev is uint8_t[n], out_dev[i] = 1 when C_i is not empty, else 0. The traversal of
 *   a plane ends at the first crossed triangle.
 * mode BM_PLANES_LIST: a CSR fill by BM_BOXES_LIST's rules. offsets_dev is uint32_t[n + 1], ascending. At
 *   least one of ids_dev and segs_dev is not null; slot j of plane i goes to ids_dev[offsets_dev[i] + j]
 *   (the triangle's global id) and/or segs_dev[offsets_dev[i] + j] (a, the id, b, and the plane's index i, so
 *   the flat array is self-contained), at most offsets_dev[i+1] - offsets_dev[i] slots; nothing is ever
 *   written outside a plane's own segment, and the unused tail of a segment is left untouched. out_dev may
 *   be NULL; otherwise it is uint32_t[n] and out_dev[i] = |C_i|. The order inside a segment is the
 *   traversal's: the same for every call on the same build, on every GPU and grid size (nothing is decided
 *   by an atomic), and otherwise unspecified. A segment that is too short holds the first entries of it.
 * Invalid planes (a non-finite component of point or normal; a normal of all zeros) are not looked up:
 *   count 0, byte 0, nothing listed. The pad words are ignored. Over an empty built scene every count and
 *   byte is 0.
 * The bit-for-bit guarantee holds while no operation in s (the three differences, the three products, the two
 *   additions) overflows over the scene's bounding box; beyond that the result is unspecified (and
 *   memory-safe).
 * Precondition: positions uploaded to a mesh since the last build or refit need a refit (or build) first —
 *   the tree bounds the positions it was made from, the query reads the current ones.
 *   BM_ERROR_NOT_BUILT when the scene's meshes or their index counts are no longer the build's, as for
 *   bm_scene_hit_attributes.
 * flags: none defined yet, pass 0. Planes are taken in the order given, 16 consecutive planes per wave.
 * BM_ERROR_INVALID_PARAMETER: a null handle; with n > 0 a null planes_dev, a null out_dev unless the mode is
 * BM_PLANES_LIST, with BM_PLANES_LIST a null offsets_dev or both of ids_dev and segs_dev null; a misaligned
 * pointer; an unknown mode or flag bit; a scene of a reference-mode, BVH2 or BVH8 context.
 * BM_ERROR_NOT_BUILT: the scene has no current build. n = 0 succeeds without a launch. */
typedef struct bm_plane {
    float point[3];
    uint32_t pad0;
    float normal[3];
    uint32_t pad1;
} bm_plane; /* 32 B */
typedef struct bm_segment {
    float a[3];
    uint32_t tri_id;
    float b[3];
    uint32_t plane;
} bm_segment; /* 32 B */
#define BM_PLANES_COUNT 0u
#define BM_PLANES_ANY 1u
#define BM_PLANES_LIST 2u
int32_t bm_scene_section_planes(bm_scene* s, const bm_plane* planes_dev, uint32_t n, uint32_t mode, uint32_t flags,
                                void* out_dev, const uint32_t* offsets_dev, uint32_t* ids_dev, bm_segment* segs_dev);
/* The counting build of the same query: out[0] BVH node records fetched, out[1] triangle tests (a leaf's
 * triangle count per leaf reached), out[2] the sum of |C_i| (BM_PLANES_ANY: the number of planes with a
 * crossing), out[3] the largest number of stack entries any plane held at once (above 24 the traversal used
 * the global overflow area); invalid planes count nothing. Results are written exactly as
 * bm_scene_section_planes writes them. Synchronous. */
int32_t bm_scene_section_planes_counters(bm_scene* s, const bm_plane* planes_dev, uint32_t n, uint32_t mode,
                                         uint32_t flags, void* out_dev, const uint32_t* offsets_dev,
                                         uint32_t* ids_dev, bm_segment* segs_dev, uint64_t out[4]);

/* ---- hit attributes: the meshes' vertex slots interpolated at ray-query hits ------------------
 * The reference's bmFaceInterpolate<T>(face, u, v, meshData, dataIdx) (CudaComon.cuh:253-266) over n
 * bm_hit records in device memory (as bm_scene_trace_rays writes them, or made by the caller): what a
 * caller needs to shade or to start the next ray from, without mirroring the meshes itself.
 * For hit i with tri_id = g: the scene mesh m and its face f with tri_offset[m] <= g < tri_offset[m] +
 * num_tris[m] (global ids as bm_scene_build defines them), the indices idx[3f .. 3f+2] of mesh m, the
 * vertices a0, a1, a2 of the requested slot there, and per component, in float32 without contraction,
 *     w = 1.f - (u + v);  out = (a0 * w + a1 * u) + a2 * v
 * (the trace's own normal interpolation). BM_ATTR_NORMALIZE (3-component requests) multiplies every
 * component by 1.f / sqrtf((x*x + y*y) + z*z).
 * Pseudo-slots: BM_ATTR_GEOM_NORMAL: with e1 = v1 - v0, e2 = v2 - v0 of the position slot,
 *   (e1.y*e2.z - e2.y*e1.z, e1.z*e2.x - e2.z*e1.x, e1.x*e2.y - e2.x*e1.y), normalised on request;
 *   BM_ATTR_MESH_FACE: the uint32 pair {m, f}.
 * Misses: a record whose tri_id is BM_NO_TRIANGLE, or >= the built triangle count, is not looked up: its
 *   rows are zeros, {0xFFFFFFFF, 0xFFFFFFFF} for BM_ATTR_MESH_FACE. Only tri_id ever indexes memory; u and
 *   v are used as given (a non-finite u or v propagates arithmetically).
 * Mixed scenes: every mesh that has the requested slot must have `components` components there and at
 *   least one mesh of the scene must have it, else BM_ERROR_INVALID_FORMAT (a scene without meshes has
 *   only misses and accepts any slot); hits on a mesh without the slot get zero rows (NORMALIZE or not).
 * The values read are the meshes' device buffers when the kernel runs: a bm_mesh_set_vertex_data after
 *   the build is seen without a rebuild (positions and normals after a bm_scene_refit likewise). The
 *   mesh set and the triangle counts must be those of the last build or refit (bm_scene_refit's own
 *   comparison), else BM_ERROR_NOT_BUILT; every mesh's largest index must be below its vertex count at
 *   call time, else BM_ERROR_INVALID_PARAMETER.
 * 1..BM_ATTR_MAX_REQS requests are served by one launch that finds the mesh and loads the indices once
 *   per hit; the result is bit-identical to one call per request. hits_dev and every out_dev are device
 *   pointers on the context's device, 16-byte aligned; out_dev receives n rows of `components` 4-byte
 *   words, tightly packed. The work is enqueued on the context stream (after earlier builds and ray
 *   queries) and the call returns without waiting; repeated calls over unchanged meshes do not
 *   synchronise with the device. On a multi-device context it runs on the root device alone.
 * BM_ERROR_INVALID_PARAMETER: a null handle or request array, null hits_dev or out_dev with n > 0, a
 *   misaligned hits_dev or out_dev, num_reqs 0 or > BM_ATTR_MAX_REQS, an unknown slot or flag bit,
 *   components outside 1..4 (BM_ATTR_GEOM_NORMAL: 3, BM_ATTR_MESH_FACE: 2), BM_ATTR_NORMALIZE on a
 *   request that is not 3-component or is BM_ATTR_MESH_FACE, non-zero pad, a scene of a reference-mode,
 *   BVH2 or BVH8 context (bm_hit records only come from BVH4 scenes; the kernel does not read the BVH).
 * BM_ERROR_NOT_BUILT: no current build. n = 0 succeeds without a launch. */
#define BM_ATTR_GEOM_NORMAL 16u /* pseudo-slot: cross(v1-v0, v2-v0) of the position slot, 3 floats, unnormalised */
#define BM_ATTR_MESH_FACE 17u   /* pseudo-slot: uint32 {scene mesh index, face index within it}, 2 words */
#define BM_ATTR_NORMALIZE 1u    /* flags: 3-component requests only; v * (1.f / sqrtf(dot(v,v))) */
#define BM_ATTR_MAX_REQS 4u
typedef struct bm_attr_req {
    uint32_t slot;       /* BM_VERTEX_DATA_* or a BM_ATTR_* pseudo-slot */
    uint32_t components; /* floats per output row: 1..4 (GEOM_NORMAL 3, MESH_FACE 2) */
    uint32_t flags;      /* BM_ATTR_* bits */
    uint32_t pad;        /* 0 */
    void* out_dev;       /* n rows of `components` 4-byte words, tightly packed; 16-byte aligned base */
} bm_attr_req;           /* 24 B */
int32_t bm_scene_hit_attributes(bm_scene* s, const bm_hit* hits_dev, uint32_t n, const bm_attr_req* reqs,
                                uint32_t num_reqs);

/* ---- instance transforms: place a mesh many times, move it by refit -----------------------------
 * The reference has no transforms: its Model::load can add one mesh numAdds times, every copy on the same
 * spot. bm_scene_add_instance adds "this mesh, at this 3x4 matrix" as one more entry of the scene's list.
 * A transform is 12 floats, row-major 3x4: element (r, c) is xform[4*r + c], the linear part
 * L[r][c] = xform[4*r + c] (c < 3), the translation xform[4*r + 3] — the layout of VkTransformMatrixKHR,
 * OptiX and Embree.
 * Flattened instancing: every instance entry gets its own triangle records, as every added mesh does. The
 * scene owns world-space copies of an instance's positions and normals, written by one kernel launch on the
 * context stream at the start of every bm_scene_build and bm_scene_refit (inside build_ms); the build reads
 * those instead of the mesh's own slots. A scene without instance entries enqueues exactly what it did before.
 * Entries and indices: an entry's position in the list (plain entries of bm_scene_add_mesh and instance
 *   entries counted alike, in the order added) is its index: the m that BM_ATTR_MESH_FACE reports, and the
 *   order in which global triangle ids are assigned. Removing an earlier entry shifts later ones down by one.
 *   A mesh may be added any number of times, as a plain entry and as an instance alike.
 * Arithmetic, float32, one rounding per operation in the order written, never contracted into fused
 *   multiply-adds (results are reproducible bit for bit by the same statements in any IEEE float32):
 *     position  p'[r] = ((x[4r]*p.x + x[4r+1]*p.y) + x[4r+2]*p.z) + x[4r+3]            r = 0, 1, 2
 *     normal    n'[r] = (C[r][0]*n.x + C[r][1]*n.y) + C[r][2]*n.z
 *   C is the cofactor matrix of L (its inverse transpose times its determinant), computed on the host by
 *   bm_xform_normal_matrix, which the build itself calls:
 *     c00 = L11*L22 - L12*L21   c01 = L12*L20 - L10*L22   c02 = L10*L21 - L11*L20
 *     c10 = L02*L21 - L01*L22   c11 = L00*L22 - L02*L20   c12 = L01*L20 - L00*L21
 *     c20 = L01*L12 - L02*L11   c21 = L02*L10 - L00*L12   c22 = L00*L11 - L01*L10
 *   Normals are not renormalised and their sign is not fixed up for mirroring matrices (det L < 0 flips
 *   them): the trace normalises after interpolation, and interpolation commutes with a linear map. A singular
 *   matrix is accepted; it makes degenerate triangles, as a caller's own vertices can.
 * Hit attributes (bm_scene_hit_attributes): BM_VERTEX_DATA_POSITION, BM_VERTEX_DATA_NORMAL and
 *   BM_ATTR_GEOM_NORMAL of a hit on an instance entry are in world space, as of the last build or refit
 *   (a bm_mesh_set_vertex_data of positions or normals after it is not seen before the next one). Every other
 *   slot — UVs, TANGENT, BITANGENT, the EXTRAs — is the mesh's own, as uploaded: BM_ATTR_MESH_FACE's m with
 *   bm_scene_get_instance_transform and bm_xform_normal_matrix give a caller what it needs to transform
 *   tangents itself. An instance whose mesh now indexes vertices past the vertex count of that build or refit
 *   gives BM_ERROR_NOT_BUILT.
 * On a multi-device context every replica transforms its own copy. Works with BVH4, BVH2 and both reference
 * modes; bm_scene_refit's "same meshes, same triangle counts" rule is unchanged.
 * Errors of the calls below: BM_ERROR_INVALID_PARAMETER for a null handle or matrix, a non-finite matrix
 * element, an index past the list, a mesh of another context. */
/* Appends an instance entry and marks the scene unbuilt, as bm_scene_add_mesh does; *index_out (may be NULL)
 * receives the entry's index. */
int32_t bm_scene_add_instance(bm_scene* s, bm_mesh* m, const float xform[12], uint32_t* index_out);
/* Replaces the entry's matrix; launches nothing and does not mark the scene unbuilt. The new placement takes
 * effect at the next bm_scene_build or bm_scene_refit; until then traces, ray queries and hit attributes all
 * see the old one. index must name an entry made by bm_scene_add_instance. Rigid animation is this call per
 * moved object plus one bm_scene_refit. */
int32_t bm_scene_set_instance_transform(bm_scene* s, uint32_t index, const float xform[12]);
/* The matrix last set for an instance entry (not necessarily the one of the last build); a plain entry is
 * BM_ERROR_INVALID_PARAMETER. */
int32_t bm_scene_get_instance_transform(const bm_scene* s, uint32_t index, float xform_out[12]);
/* Erases the entry at index, plain or instance, and marks the scene unbuilt. bm_scene_remove_mesh keeps its
 * behaviour: it erases the first entry whose mesh is m, of either kind. */
int32_t bm_scene_remove_instance(bm_scene* s, uint32_t index);
/* The cofactor matrix C above, row-major 3x3, of xform's linear part. Host only: no context, no device. */
int32_t bm_xform_normal_matrix(const float xform[12], float out9[9]);

/* ---- camera: ICamera (Beam.h:65-72, Camera.cpp) ----------------------------------------- */
int32_t bm_camera_create(bm_context* ctx, bm_camera** out);
/* setInitialRays (Camera.cpp:43-72): same sequential ray recurrence and validation. */
int32_t bm_camera_set_initial_rays(bm_camera* c, uint32_t width, uint32_t height, float left,
                                   float right, float top, float bottom, float zoom);
/* traceScene (Camera.cpp:85-97 -> SceneTree::march -> bmMarch): one primary ray per pixel,
 * eye[3], orient_colmajor[9] (glm mat3 memory layout). The render target's size must equal the
 * camera's (Scene.cpp:81-97, BM_ERROR_RT_CAM_MISMATCH). On a multi-device context (bm_options
 * devices / comm_*) the frame's bands are traced on every device and gathered into the target;
 * bm_camera_trace_shadow likewise. The band, counter and profile entry points below run on the
 * root device alone.
 * Range: frames and ray queries (bm_scene_trace_rays) equal the exhaustive trace over all triangles for
 * any world offset, uniform scales 2^-30 .. 2^30 and ray origins within 32 scene extents of the scene's
 * box. Beyond that they equal the oracle's BVH traversal and differ from the exhaustive trace on a
 * measured share of the pixels (2 of 295,000 at 64 extents, about 1 in 1,000 at 32,768).
 * A pixel or record carries a triangle id exactly when its t is finite and positive, at any scale. */
int32_t bm_camera_trace(bm_camera* c, const float* eye3, const float* orient3x3, bm_scene* s,
                        bm_rt* rt);
/* Screen-band partition for multi-GPU: trace only global rows in bands b*band_height..+band_height
 * with b % band_step == band_first, writing them compacted into rt (local row r holds global row
 * ((r/band_height)*band_step + band_first)*band_height + r%band_height). rt width must equal the
 * camera width and its height must be >= the compacted row count. band_step=1, band_first=0 is
 * bm_camera_trace. */
int32_t bm_camera_trace_bands(bm_camera* c, const float* eye3, const float* orient3x3, bm_scene* s,
                              bm_rt* rt, uint32_t band_height, uint32_t band_step,
                              uint32_t band_first);
/* Primary trace plus one shadow ray per hit toward a point light (the reference
 * has no shadow rays, so the semantics are this build's): origin = eye + dir * (t * 0.9999f),
 * direction = light3 - origin (unnormalised); the pixel's shadow-plane byte is 1 when any triangle's
 * Möller-Trumbore t_s has 0 < t_s < 1 (any hit), else 0 (also on a primary miss). The primary
 * planes are written exactly as bm_camera_trace writes them; read the shadow plane with
 * bm_rt_read_shadow / bm_rt_shadow. Hit pixels are compacted into a queue on the device (wave64
 * ballots) and the shadow rays run as a second persistent pass over it. */
int32_t bm_camera_trace_shadow(bm_camera* c, const float* eye3, const float* orient3x3, bm_scene* s,
                               bm_rt* rt, const float* light3);
/* bm_camera_trace_bands + the shadow pass over the band's rows. */
int32_t bm_camera_trace_shadow_bands(bm_camera* c, const float* eye3, const float* orient3x3,
                                     bm_scene* s, bm_rt* rt, uint32_t band_height,
                                     uint32_t band_step, uint32_t band_first, const float* light3);
void bm_camera_destroy(bm_camera* c);

/* ---- render target: IRenderTarget (Beam.h:32-45) — offscreen device planes --------------- */
/* Replaces registerGLTBO (RenderTarget.cpp:17-28): device planes owned by the library.
 * pitch (bytes per row of the packed plane) >= width*4, 0 = width*4. */
int32_t bm_rt_create_offscreen(bm_context* ctx, uint32_t width, uint32_t height, uint32_t pitch,
                               bm_rt** out);
/* Wrap caller-owned device memory (e.g. torch tensors): packed (pitch*height bytes), tri_id and t
 * (width*height each) are required, nz (width*height floats, |n.z| of the shading normal) may be
 * NULL. */
int32_t bm_rt_create_external(bm_context* ctx, uint32_t width, uint32_t height, uint32_t pitch,
                              void* packed, void* tri_id, void* t, void* nz, bm_rt** out);
uint32_t bm_rt_width(const bm_rt* rt);
uint32_t bm_rt_height(const bm_rt* rt);
uint32_t bm_rt_pitch(const bm_rt* rt);
/* Device pointers of the planes (IRenderTarget::buffer() is the packed plane). */
void* bm_rt_buffer(const bm_rt* rt);
void* bm_rt_tri_id(const bm_rt* rt);
void* bm_rt_t(const bm_rt* rt);
void* bm_rt_nz(const bm_rt* rt);
/* u8 shadow plane (width*height, row stride width); NULL until the first shadow trace. */
void* bm_rt_shadow(const bm_rt* rt);
/* lock/unlock keep the reference's ordering contract (RenderTarget.cpp:53-83): trace requires a
 * locked target in the C++ layer; in the C ABI the target is passed explicitly. */
int32_t bm_rt_lock(bm_rt* rt);
int32_t bm_rt_unlock(bm_rt* rt);
/* ICamera::clear / bmClear (RTClear.cu:19-48): fill the packed plane (pitch honoured). */
int32_t bm_rt_clear(bm_rt* rt, uint32_t value);
/* Synchronous readback of any subset of planes (NULL = skip). packed is width*height u32 (pitch
 * removed); rgb is width*height*3 floats: (|n.z|,0,0) on a hit, (0,1,0) on a miss. */
int32_t bm_rt_read(bm_rt* rt, uint32_t* packed, uint32_t* tri_id, float* t, float* rgb);
/* Synchronous readback of the shadow plane (width*height bytes). */
int32_t bm_rt_read_shadow(bm_rt* rt, uint8_t* out);
/* Frames in flight. A render target may carry its own HIP stream (NULL or the context stream:
 * the default). Traces into it, and its clear/readback calls, are enqueued there instead of on the
 * context stream, so traces into different targets can run concurrently (the next frame's
 * workgroups fill the CUs the previous frame's tail leaves idle). The library orders them with
 * events: a trace waits for the context stream's work (builds, ray tables) enqueued before it, and
 * a build or setInitialRays waits for the last trace of every such target. bm_sync waits for all
 * of them. Each such target owns its traversal-stack overflow area. The caller keeps the stream
 * alive while the target uses it. Not available with the global-ticket diagnostic variants. */
int32_t bm_rt_set_stream(bm_rt* rt, void* stream);
/* The stream a render target's work runs on (its own, or the context's). */
void* bm_rt_stream(const bm_rt* rt);
/* Which kernels the last trace into this target ran (measurement: names the dominant kernel). A
 * target on its own stream over a sparse view (the scene's box under half the frame) takes the
 * root cull + compacted ray quads; otherwise ray quads (BVH4) or one lane per ray. -1: no trace. */
#define BM_TRACE_KIND_QUADS 0       /* k_trace_quad */
#define BM_TRACE_KIND_CULL_QUADS 1  /* k_cull + k_trace_rays */
#define BM_TRACE_KIND_LANES 2       /* k_trace_persistent / k_trace_tiles (BVH2, shadow queue, variants) */
#define BM_TRACE_KIND_KD_MARCH 3    /* reference mode: k_kd_march_coop */
#define BM_TRACE_KIND_HASH_MARCH 4  /* hashed-grid mode: k_hash_march */
#define BM_TRACE_KIND_PACKETS 5     /* k_trace_packet (BM_PARAM_TRACE_VARIANT 14: wave packets) */
/* The distance, in largest sides of the scene's box from that box's centre, within which frames equal the
 * exhaustive trace (the range note at bm_camera_trace; measured by tests/test_oracle_range.py, whose D_OK it
 * must equal). Wave packets run for eyes within it, once the last build's box has reached the host; other
 * frames of that variant take the quad kernel. */
#define BM_ENVELOPE_EXTENTS 32
int32_t bm_rt_trace_kind(const bm_rt* rt);
/* Measurement: the ray queue of the last trace into this target, when that trace was compacted
 * (BM_TRACE_KIND_CULL_QUADS; BM_ERROR_NOT_BUILT otherwise). *regions = its queue regions; out receives the
 * first min(capacity, *regions) region counts — the rays per region that survived k_cull and were traced
 * as quads (their sum: the queue's rays; k_trace_rays walks ceil(sum / 16) batches). Synchronous. */
int32_t bm_rt_ray_queue_counts(bm_rt* rt, uint32_t* out, uint32_t capacity, uint32_t* regions);
/* Multi-device contexts: the device-time split of the last frame traced into this (root) target,
 * from HIP events on the streams it ran on: out_ms[0] = this process's band trace (its first band
 * source), out_ms[1] = the exchange after it (RCCL send/recv or peer writes, band scatter and
 * reshade; on rank 0 it includes waiting for the slowest rank's bands). Synchronous: waits for
 * that frame. BM_ERROR_NOT_BUILT before the first multi-device trace into rt. */
int32_t bm_rt_last_timing(bm_rt* rt, float out_ms[2]);
/* Host dump of the packed plane as a binary PPM (P6, 8-bit R,G,B from 0x00RRGGBB, rows top to
 * bottom): the frame-loop step after trace that the reference hands to GL (SURVEY 8(f)2,
 * Program.cpp:314-341). Synchronous; BM_ERROR_INVALID_PARAMETER if the file cannot be written. */
int32_t bm_rt_save_ppm(bm_rt* rt, const char* path);
void bm_rt_destroy(bm_rt* rt);

/* ---- self-test --------------------------------------------------------------------------------
 * The trace kernels' scalar primitives on n host records, run on the context's device (synchronous):
 * orient*ray, 1/dir, Möller-Trumbore (bmTriIntersect, CudaComon.cuh:117-155, with the trace's
 * exact-safe early reject), interpolate + normalize + pack (CudaComon.cuh:253-266, BuildTree.cu:
 * 489-491). in: 36 floats per record (orig[3] ray[3] orient[9, column-major] v0[3] v1[3] v2[3]
 * n0[3] n1[3] n2[3] su sv pad); out: 12 floats (dir[3] 1/dir[3] t u v — t = FLT_MAX and u = v = 0 on
 * a reject — packed colour bits, normalised n.z, pad). tests/test_gpu_glm_pin.py compares them bit
 * for bit with the reference's glm 0.9.9.0 (tests/golden/glm_pin.npz). */
int32_t bm_debug_primitives(bm_context* ctx, uint32_t n, const float* in, float* out);
/* Test hook of the cost-ordered schedule (BM_PARAM_TRACE_SCHED 2): the table of 10-ns tick counts per 4x4
 * quad-kernel tile that each trace of this target records and the next one sorts its tiles by. set (non-null):
 * the table is made to hold at least n words and the n host words are copied in on the target's stream; the
 * next trace uses them as given (no zero fill). get (non-null): n words are copied out once the stream's work
 * has completed (after the set, when both are given; BM_ERROR_NOT_BUILT when the table holds fewer).
 * Synchronous. BM_ERROR_INVALID_PARAMETER for a multi-device context, n == 0 or both pointers null.
 * tests/test_gpu_tile_order.py traces injected tables against the oracle. */
int32_t bm_rt_debug_tile_costs(bm_rt* rt, uint32_t n, const uint32_t* set, uint32_t* get);

/* ---- OBJ ingest: TestProgram's Model::load (TestProgram/Model.cpp:26-126) without Assimp ------ */
/* Host-side parse (no device work): one mesh per material run (a `usemtl` after faces, or `o`/`g`,
 * starts a new mesh), file face order, polygons as fans (0,j,j+1), corners with equal (v,vt,vn)
 * index triples shared in first-use order, normals vn[ni] and UV1 vt[ti] when every corner has
 * them; for meshes with both, the tangent space Model.cpp:34 asks Assimp for (aiProcess_CalcTangentSpace,
 * restated in bm_obj.cpp: per-corner face tangents projected into the normal's plane, smoothed over
 * corners at the same position within 45 degrees) into slots BM_VERTEX_DATA_TANGENT/BITANGENT, corners
 * with different tangents not sharing a vertex. Floats parsed with strtof. BM_ERROR_INVALID_PARAMETER if the file cannot be opened,
 * BM_ERROR_INVALID_FORMAT on a malformed face. */
#define BM_OBJ_UNSHARED 1u /* one vertex per corner instead of sharing equal index triples */
typedef struct bm_model bm_model;
typedef struct bm_model_info {
    uint32_t num_meshes;
    uint64_t num_faces;
    uint64_t num_vertices;
    float bmin[3], bmax[3]; /* over the referenced positions (Model.cpp:69-79, 119-122) */
} bm_model_info;
int32_t bm_model_load(const char* path, uint32_t flags, bm_model** out);
int32_t bm_model_info_get(const bm_model* m, bm_model_info* info);
/* Host arrays of mesh i (valid until bm_model_destroy); nrm/uv are NULL when absent. */
int32_t bm_model_mesh(const bm_model* m, uint32_t i, const float** pos, const float** nrm, const float** uv,
                      const uint32_t** idx, uint32_t* num_vertices, uint32_t* num_indices,
                      const char** material);
/* Model::load's upload (Model.cpp:49-114): create one bm_mesh per mesh on ctx (once) and, when
 * scene is non-NULL, add each to it num_adds times. The meshes belong to the model: remove them
 * from scenes (or destroy the scenes) before bm_model_destroy. */
int32_t bm_model_upload(bm_model* m, bm_context* ctx, bm_scene* scene, uint32_t num_adds);
/* The same upload (once per model), then every mesh added to scene as an instance entry with the one
 * matrix (bm_scene_add_instance), in mesh order. */
int32_t bm_model_add_instance(bm_model* m, bm_context* ctx, bm_scene* scene, const float xform[12]);
/* Tangents and bitangents of mesh i (3 floats per vertex), NULL when the mesh has no normals or no UVs. */
int32_t bm_model_mesh_tangents(const bm_model* m, uint32_t i, const float** tangent, const float** bitangent);
bm_mesh* bm_model_gpu_mesh(const bm_model* m, uint32_t i);
void bm_model_destroy(bm_model* m);

/* ---- measurement ------------------------------------------------------------------------- */
/* Re-trace the camera view with the counting build of the trace kernel and return the totals
 * over all pixels: out[0] BVH node records fetched, out[1] triangle tests, out[2] hits. Output
 * planes are written exactly as bm_camera_trace writes them. Synchronous. */
int32_t bm_camera_trace_counters(bm_camera* c, const float* eye3, const float* orient3x3,
                                 bm_scene* s, bm_rt* rt, uint64_t out[3]);
/* Counting build of bm_camera_trace_shadow: out[0..2] as above for the primary rays, out[3] node
 * records and out[4] triangle tests of the shadow rays, out[5] shadowed pixels. Synchronous. */
int32_t bm_camera_trace_shadow_counters(bm_camera* c, const float* eye3, const float* orient3x3,
                                        bm_scene* s, bm_rt* rt, const float* light3, uint64_t out[6]);
/* Diagnostic trace (same outputs) recording, per wave64 of the persistent launch, four u64: start
 * and end s_memrealtime (100 MHz), (XCC id << 32 | HW_ID), and the sum over the wave's 8x8 tiles of
 * each tile's longest per-lane work (node records + triangle tests). per_wave holds 4*max_waves
 * u64; *num_waves receives the waves launched, or the capacity needed when max_waves is too small
 * (then BM_ERROR_INVALID_PARAMETER). Synchronous; never used for timing. */
int32_t bm_camera_trace_profile(bm_camera* c, const float* eye3, const float* orient3x3, bm_scene* s,
                                bm_rt* rt, uint64_t* per_wave, uint32_t max_waves,
                                uint32_t* num_waves);
/* Export the built BVH for structural parity tests (synchronous; any pointer may be NULL):
 * records[num_records*16] u32, tris[num_tris*12] u32 (sorted order), keys[num_tris] sorted
 * Morton keys, perm[num_tris] sorted position -> global triangle id. */
int32_t bm_scene_export(bm_scene* s, uint32_t* records, uint32_t* tris, uint32_t* keys,
                        uint32_t* perm);
/* For tests: bm_mesh_compute_normals' kernel over the caller's own device buffers, on the context stream, so
 * that a test can supply the vertex -> corner table and look behind the last row written. pos_dev: 3 * nv
 * floats; idx_dev: the indices; table_dev: nv + 1 row offsets, then the corner ids sorted by vertex (every id
 * below the number of indices, every index below nv: the caller's duty, nothing is checked); nrm_dev receives
 * 3 * nv floats. flags as bm_mesh_compute_normals. BM_ERROR_INVALID_PARAMETER for a null context or, with
 * nv > 0, a null pos_dev, table_dev or nrm_dev, and for an unknown flag bit. Asynchronous. */
int32_t bm_debug_vertex_normals(bm_context* ctx, const float* pos_dev, const uint32_t* idx_dev,
                                const uint32_t* table_dev, float* nrm_dev, uint32_t nv, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* BEAM_C_H */
