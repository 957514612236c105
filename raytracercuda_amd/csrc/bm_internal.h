// bm_internal.h — launch interface between the C-ABI layer (bm_api.cpp) and the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/beam_c.h"
#include "bm_common.h"

// A/B builds (tools/build_ab.py ... BM_TRACE_AB=1) add the trace variants measured slower than the
// product kernels (bm_trace_ab.hip) and BVH8; the in-tree library is built without them.
#ifndef BM_TRACE_AB
#define BM_TRACE_AB 0
#endif

namespace bm {

// A context's tuning parameters (bm_context_set_param, BM_PARAM_* in beam_c.h): -1 = the library
// default. Launch code reads them from here; nothing is read from the environment.
struct Tuning {
    int64_t v[BM_PARAM_COUNT];
    Tuning() {
        for (int64_t& x : v) x = -1;
    }
    int64_t get(int key, int64_t dflt) const { return v[key] >= 0 ? v[key] : dflt; }
};

// Device buffers of one acceleration-structure build (all owned by the scene, grow-only).
struct BuildBuffers {
    uint32_t n = 0;          // triangles
    uint32_t num_meshes = 0;
    uint32_t leaf_size = 4;
    uint32_t width = 4;           // BVH4 (128-B records), BVH2 (64-B) or BVH8 (256-B, from the BVH2 records)
    const MeshDesc* meshes = nullptr;
    float4* tri_orig = nullptr;   // 3n, original order (written only when need_orig: orig_records, n == 1)
    bool orig_records = false;    // the caller needs tri_orig after the build (a multi-device root's reshade)
    bool* orig_written = nullptr; // out: launch_build / launch_refit wrote tri_orig
    float* nrm = nullptr;         // 9n, original order (corner normals)
    float* aabb = nullptr;        // 6n, original order (written only when need_aabb: n == 1, non-mesh-direct)
    float* cen = nullptr;         // 3n, original order: AABB centres (the Morton keys' input)
    uint32_t* bounds = nullptr;   // build metadata block (build_meta_words(n), zero-filled per build):
                                  // BOUNDS_SLOTS bounds, gather tickets, the radix-sort counters and
                                  // histograms, then per-block partial bounds (bm_build.hip)
    uint32_t* keys = nullptr;     // n  (sorted on return)
    uint32_t* vals = nullptr;     // n  (sorted position -> global id on return)
    uint32_t* keys2 = nullptr;    // n  scratch
    uint32_t* vals2 = nullptr;    // n  scratch
    uint32_t* lch = nullptr;      // n-1
    uint32_t* rch = nullptr;      // n-1
    uint32_t* first = nullptr;    // n-1
    uint32_t* last = nullptr;     // n-1
    uint32_t* parent_leaf = nullptr;  // n
    uint32_t* parent_int = nullptr;   // n-1
    float* ibox = nullptr;            // 6(n-1): boxes of nodes whose range lies in one refit chunk
    float* pre = nullptr;             // 6n: in-chunk prefix unions of sorted leaf boxes
    float* suf = nullptr;             // 6n: in-chunk suffix unions
    float* table = nullptr;           // 6 * chunk_table_floats(n) / 6: sparse table of chunk unions
    uint32_t* records = nullptr;      // (width 8: 64, 4: 32, 2: 16) * max(n-1, 1)
    uint32_t* records2 = nullptr;     // width 8 only: the BVH2 records it is collapsed from (16 * max(n-1, 1))
    float4* tris = nullptr;           // 3n, sorted order
    // the gather's bound replicas in `bounds` are already zero (the previous LBVH build or refit of
    // this buffer cleared them after their last reader): launch_build / launch_refit skip the memset
    bool replicas_clean = false;
    const Tuning* tune = nullptr;  // the context's parameters (BM_PARAM_MSD_*, NRM_DEFER, BUCKET_LDS_CAP)
};

size_t build_meta_words(uint32_t n);
// largest top-digit-first sort: the device-side LSD fallback's last pass runs in RADIX (1,024) bucket
// workgroups of one tile each, i.e. at most 1,024 top-digit tiles (2^22 keys take 512)
constexpr uint32_t MSD_MAX_N_CAP = 1u << 22;
bool msd_sort(uint32_t n, const Tuning& t);  // launch_build sorts the top digit first, then each bucket
uint32_t build_sort_skew_word();             // meta word: nonzero when that sort fell back to LSD passes
size_t chunk_table_floats(uint32_t n);
uint32_t num_records(uint32_t n);
hipError_t launch_build(const BuildBuffers& b, hipStream_t s);
// Refit: new triangle data and boxes over the topology (vals, tree arrays) of the last launch_build
// with the same buffers and triangle count.
hipError_t launch_refit(const BuildBuffers& b, hipStream_t s);

// Triangle records (original order), corner normals and AABBs only (reference modes: no scene bounds);
// zeroes b.bounds words 0 and 1 (the reference-mode split descent keeps its queue count and overflow
// flag there, so the count pass needs no fill launch).
hipError_t launch_gather(const BuildBuffers& b, hipStream_t s);
// The original-order triangle records only (b.meshes, b.num_meshes, b.n, b.tri_orig): for a reshade
// after a build that did not write them (need_orig false at build time).
hipError_t launch_orig_records(const BuildBuffers& b, hipStream_t s);
#ifdef BM_BUILD_DIAG
hipError_t build_diag(unsigned long long* out);     // diagnostic builds: per-wave slots, LBVH build rows (bm_build.hip)
hipError_t kd_build_diag(unsigned long long* out);  // the same, kd build rows (bm_kd.hip)
#endif

// Readback of na words at a and nb at b (na + nb < POST_SEQ_WORD) into pinned coherent host memory
// `host` (device view), then `seq` released into host[POST_SEQ_WORD] (bm_api.cpp readback spins on it).
constexpr uint32_t POST_SEQ_WORD = 63;
hipError_t launch_post(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb, uint32_t* host, uint32_t seq,
                       hipStream_t s);

// Generic stable sort of (key, value) u32 pairs on the low key_bits bits (10-bit one-sweep passes).
// smeta: sort_meta_words(n, key_bits) words of scratch. *in_scratch: the result is in keys2/vals2.
// topmap (31-bit keys only): a 2,048-bit map of the values of bits 20-30 present (at most 1,024 set):
// three passes, the last on the rank of those bits (bm_build.hip build_top_rank) — the same order.
size_t sort_meta_words(uint32_t n, int key_bits);
constexpr uint32_t KD_TOPMAP_WORDS = 64;  // 2,048 bits
hipError_t launch_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys2, uint32_t* vals2, uint32_t n,
                             int key_bits, uint32_t* smeta, hipStream_t s, bool* in_scratch, bool meta_zeroed = false,
                             const uint32_t* topmap = nullptr);
// Karras radix tree over n sorted keys (equal keys: position tiebreak), as in the BVH build.
hipError_t launch_radix_tree(const uint32_t* keys, uint32_t n, uint32_t* lch, uint32_t* rch, uint32_t* first,
                             uint32_t* last, uint32_t* parent_leaf, uint32_t* parent_int, hipStream_t s,
                             const uint32_t* n_dev = nullptr);

// Trace kernel variants (LDS stack depth / overflow policy / grid shape); the C ABI picks one per
// context (BM_TRACE_VARIANT overrides it for A/B measurements).
enum TraceVariant {
    TRACE_TILES_SCRATCH16 = 0,   // 16x16 tile per workgroup, LDS stack 16, scratch overflow
    TRACE_TILES_NOOVF16 = 1,     // experiment only: no overflow (drops beyond 16 entries)
    TRACE_PERSIST_GLOBAL16 = 2,  // persistent waves over 8x8 tiles, LDS 16, global overflow
    TRACE_PERSIST_GLOBAL8 = 3,
    TRACE_PERSIST_GLOBAL12 = 4,
    TRACE_PERSIST_DIAG12 = 5,    // diagnostic: PRIO12 + per-wave timestamps (bm_camera_trace_profile only)
    TRACE_PERSIST_PRIO12 = 6,    // persistent LDS 12 + s_setprio boost of long-running waves
    TRACE_PERSIST_PRIO8 = 7,     // persistent LDS 8 + the same boost
    TRACE_PERSIST_DYN12 = 8,     // persistent LDS 12 + boost, tiles taken dynamically (atomic ticket)
    TRACE_PERSIST_DYN16 = 9,
    TRACE_QUAD = 10,             // persistent, four lanes per ray over the BVH4 (4x4 pixel tile per wave)
    TRACE_QUAD_FETCH = 11,       // ray quads + in-wave ray refill (idle quads take the wave's next rays)
    TRACE_COMPACT = 12,          // lane-per-ray setup + root cull and ray queue, then quads over the survivors
    TRACE_PAIR = 13,             // persistent, two lanes per ray over the BVH4 (8x4 pixel tile per wave)
    TRACE_PACKET = 14,           // wave packets: one 8x8 tile per wave, wave-uniform stack, scalar record loads
    TRACE_NUM_VARIANTS
};
// Traversal stack bound: a Karras tree over 30-bit keys + 32-bit position tiebreak is < 64 levels
// deep; BVH2 pushes at most one entry per level, BVH4 (half the levels) at most three.
constexpr int MAX_STACK = 96;
constexpr int MAX_STACK8 = 160;  // BVH8: up to 7 pushes per node step

struct TraceParams {
    const uint4* nodes;          // records as 4 x uint4 (BVH2) or 8 x uint4 (BVH4)
    const float4* tris;          // sorted triangle records
    const float* nrm;            // 9 per original triangle
    const float* rx;             // camera column table (W)
    const float* ry;             // camera row table (H)
    float z2, zoom;
    float eye[3];
    float orient[9];             // column-major glm mat3
    uint32_t width, height;      // full frame
    uint32_t band_h, band_step, band_first;
    uint32_t local_rows;         // rows present in the render target
    uint32_t pitch_u32;          // packed-plane row stride (u32 elements)
    uint32_t num_tris;           // 0 -> every pixel misses
    uint32_t* packed;
    uint32_t* tri_id;
    float* t;
    float* nz;
    unsigned long long* counters;  // [3], counting build only
    uint32_t* ovf_ref;             // global stack overflow [MAX_STACK - lds][ovf_stride]
    float* ovf_t;
    uint32_t ovf_stride;           // = persistent_blocks * 256
    uint32_t persistent_blocks;    // upper bound of a persistent grid (each launch: min with residency)
    uint32_t scramble;             // persistent grid: scrambled tile order
    uint32_t prio_after;           // priority-boost variants: traversal steps before s_setprio
    uint32_t prio_level;
    uint32_t refill_min;           // quad-fetch variant: idle quads (of 16) that trigger a refill
    uint32_t sched;                // quad variant: 0 static tile order, 1 block-dynamic (LDS ticket),
                                   // 2 block-dynamic, longest first by the last trace's tile times
    uint32_t* tile_cost;           // sched 2: per quad-kernel tile, 10-ns ticks of its last trace (render target)
    int variant;
    uint32_t bvh_width;            // 2 or 4 (the scene's record layout)
    unsigned long long* tile_ctr;  // dynamic variants: monotonic ticket counter of the context
    unsigned long long tile_base;  // its value when this launch starts (tickets = tiles + waves)
    unsigned long long* diag;      // [4 per wave of the persistent grid], diagnostic build only
    // shadow rays (null shadow: primary rays only). Fused: the primary kernel traces each hit's
    // shadow ray itself. Queue (shadow_queue): the primary kernel zeroes the shadow plane and appends
    // every hit pixel (local index lr*width + x) to queue; k_shadow_persistent drains it.
    uint8_t* shadow;
    bool shadow_queue;
    uint32_t* queue;
    uint32_t* queue_count;
    float light[3];
    unsigned long long* shadow_counters;  // [3], counting build only
    // compacted variant (TRACE_COMPACT): rays that enter the root, region r at rayq + r * rayq_region
    // (x | local row << 16), rayq_count[r] of them; a region = rayq_tpr consecutive 8x8 tiles
    uint32_t* rayq;
    uint32_t* rayq_count;
    uint32_t rayq_region, rayq_tpr, rayq_regions;
    uint32_t fast_cull;  // orient is near-orthonormal: k_cull may use approximate ray setup
    uint32_t cull_depth;  // 1: k_cull tests the root record; 2: the entered child records too (BM_PARAM_CULL_DEPTH)
    // ray queries (bm_rays.hip): q_n caller rays of two float4 each, (origin, tmax) (dir, pad); q_out one
    // bm_hit (closest) or one byte (any hit) per ray. Closest-point queries (bm_points.hip): q_n points of
    // one float4 each, (p, rmax); q_out one bm_hit per point
    const float4* q_rays;
    void* q_out;
    uint32_t q_n;
    // multi-hit ray queries (bm_multihit.hip): q_out holds q_k bm_hit records per ray; q_counts (may be null
    // unless every crossing is counted) one count per ray. Multi-result point queries (bm_points_multi.hip):
    // the same two per point
    uint32_t q_k;
    uint32_t* q_counts;
    // ray query filters (bm_trace_quad.h RayFilter): the call's BM_RAYS_* filter bits (0: the unfiltered
    // kernels) and, for BM_RAYS_PAD_MASK, the owner table of the last build: q_ent_n entries that own
    // triangles, q_ent[i] the first global id of entry i (ascending), q_ent[q_ent_n + i] its mask
    uint32_t q_flags;
    uint32_t q_ent_n;
    const uint32_t* q_ent;
};

bool trace_variant_persistent(int variant);
// The product kernels (TRACE_QUAD, TRACE_COMPACT, the single-lane PRIO12 and its DIAG12 build); the
// other variants and BVH8 exist only in A/B builds (-DBM_TRACE_AB=1, bm_trace_ab.hip).
bool trace_variant_product(int variant);
bool trace_variant_built(int variant);  // compiled into this library
#if BM_TRACE_AB
hipError_t launch_trace_ab(const TraceParams& p, bool count, int shadow_mode, hipStream_t s, uint32_t* grid);
#endif
// Pixel tiles of the quad kernel for a frame (one wave each): sizes the cost-ordered schedule's table.
uint32_t quad_tiles(uint32_t width, uint32_t local_rows);
// Ray-queue geometry of TRACE_COMPACT for a frame (false: the frame does not fit its 16-bit pixel
// coordinates; the quad kernel traces it instead).
bool trace_compact_layout(uint32_t width, uint32_t local_rows, uint32_t min_tpr, uint32_t* regions,
                          uint32_t* tiles_per_region);
uint32_t trace_variant_lds(int variant);
uint32_t trace_persistent_blocks(int variant, int device);

// *grid receives the persistent grid launched (0 for the tile kernels): a dynamic variant consumes
// tiles + 4 * grid tickets.
hipError_t launch_trace(const TraceParams& p, bool count, hipStream_t s, uint32_t* grid);
// Shadow pass over the queue the preceding launch_trace (with p.shadow set) filled.
hipError_t launch_shadow(const TraceParams& p, bool count, hipStream_t s);
// Ray query (bm_rays.hip): BM_RAYS_CLOSEST or BM_RAYS_ANY_HIT over p.q_rays on a BVH4 scene, ray quads on
// the persistent grid with the overflow area set up as for launch_trace; count: into p.counters.
hipError_t launch_query_rays(const TraceParams& p, uint32_t mode, bool count, hipStream_t s);
// Closest-point query (bm_points.hip): the nearest triangle to each of p.q_n points, one float4 (p, rmax) each
// in p.q_rays, one bm_hit each into p.q_out; BVH4 scenes, set up as for launch_query_rays. count: into
// p.counters[0..3] (node records, triangle evaluations, points with a result, the deepest stack held).
hipError_t launch_closest_points(const TraceParams& p, bool count, hipStream_t s);
// Multi-hit ray query (bm_multihit.hip): the p.q_k (t, id)-nearest hits of each of p.q_n rays into p.q_out, ray i's
// at records i * q_k ..., and per ray into p.q_counts the records that are hits or, with count_all (q_counts
// required, q_k may be 0), every triangle crossed within tmax; set up as for launch_query_rays. count: into
// p.counters[0..2] (node records, triangle tests, the sum of the per-ray counts).
hipError_t launch_query_multi(const TraceParams& p, bool count_all, bool count, hipStream_t s);
// Multi-result point query (bm_points_multi.hip): the p.q_k (dd, id)-nearest triangles within rmax of each of
// p.q_n points (one float4 (p, rmax) each in p.q_rays) into p.q_out, point i's at records i * q_k ..., and per
// point into p.q_counts the records written or, with count_all (q_counts required, q_k may be 0), every
// triangle within rmax; set up as for launch_closest_points. count: into p.counters[0..3] (node records,
// triangle evaluations, the sum of the per-point counts, the deepest stack held).
hipError_t launch_closest_points_multi(const TraceParams& p, bool count_all, bool count, hipStream_t s);
// Box overlap query (bm_boxes.hip): the triangles tri_box accepts for each of p.q_n boxes, two float4
// (centre, pad) (half, pad) each in p.q_rays; set up as for launch_closest_points. mode BM_BOXES_COUNT: one
// uint32 per box into p.q_out; BM_BOXES_ANY: one byte; BM_BOXES_LIST: the ids into p.q_counts at the
// segments p.q_ent[i] .. p.q_ent[i + 1] (q_n + 1 ascending offsets; the two fields serve here under their
// ray-query names so that TraceParams, and with it every other kernel's argument block, stays as it is) and,
// where p.q_out is not null, the counts there. count: into p.counters[0..3] (node records, triangle tests,
// the sum of the counts, the deepest stack held).
hipError_t launch_overlap_boxes(const TraceParams& p, uint32_t mode, bool count, hipStream_t s);
// Triangle overlap query (bm_tris.hip): the triangles tri_tri accepts for each of p.q_n query triangles, three
// float4 (v0, pad0) (v1, pad1) (v2, pad2) each in p.q_rays; p.q_flags the call's flags (BM_TRIS_PAD_SKIP_TRI:
// pad0 is an id never reported). Modes, outputs and counters as launch_overlap_boxes, under the same names.
hipError_t launch_overlap_triangles(const TraceParams& p, uint32_t mode, bool count, hipStream_t s);
// Sphere-cast query (bm_sweep.hip): the first contact of each of p.q_n swept spheres, two float4 (origin, tmax)
// (dir, radius) each in p.q_rays; BM_SWEEP_CLOSEST: one bm_hit each into p.q_out, BM_SWEEP_ANY: one byte. Set
// up as for launch_closest_points. count: into p.counters[0..3] (node records, triangle evaluations, sweeps
// with a result, the deepest stack held).
hipError_t launch_sweep_spheres(const TraceParams& p, uint32_t mode, bool count, hipStream_t s);
// Signed-distance / occupancy query (bm_signed.hip): for each of p.q_n points (one float4 (p, rmax) each in
// p.q_rays) the crossing parity along one or, with vote3, three fixed directions; BM_SIGNED_DISTANCE: one
// bm_hit each into p.q_out, launch_closest_points' record with the sign on t; BM_SIGNED_OCCUPANCY: one byte.
// p.q_counts, where not null, is a uint8_t[q_n] for the votes (the field serves under its multi-hit name so
// that TraceParams stays as it is). Set up as for launch_closest_points. count: into p.counters[0..3] (the
// nearest phase's node records and triangle evaluations, the parity phase's node records and triangle tests).
hipError_t launch_signed_points(const TraceParams& p, uint32_t mode, bool vote3, bool count, hipStream_t s);
// ---- hit attributes (bm_attrs.hip): vertex slots interpolated at the hits of a ray query ------------
// One entry per scene mesh, in scene order: every slot's device buffer (null: the mesh has none), so the
// table depends on the meshes alone and not on what a call requests.
struct AttrMesh {
    const uint32_t* idx;  // 3 per face
    uint32_t tri_offset;  // first global triangle id of this mesh
    uint32_t num_tris;
    const float* slot[BM_VERTEX_DATA_COUNT];
};  // 96 B
static_assert(sizeof(AttrMesh) == 96, "AttrMesh is uploaded as a byte image: no padding");
enum AttrKind : uint32_t { ATTR_SLOT = 0, ATTR_GEOM_NORMAL = 1, ATTR_MESH_FACE = 2 };
struct AttrReq {
    void* out;       // n rows of comps words
    uint32_t kind;   // AttrKind
    uint32_t slot;   // ATTR_SLOT: the vertex slot read
    uint32_t comps;  // 1..4
    uint32_t normalize;
};
struct AttrParams {
    const float4* hits;       // n bm_hit records
    uint32_t n;
    uint32_t num_tris;        // the build's triangle count: ids at or above it are misses
    uint32_t num_meshes;
    const AttrMesh* meshes;   // num_meshes entries
    const uint32_t* offsets;  // their tri_offset again, packed for the search
    uint32_t num_reqs;        // 1..BM_ATTR_MAX_REQS
    AttrReq req[BM_ATTR_MAX_REQS];
};
hipError_t launch_hit_attrs(const AttrParams& p, hipStream_t s);

// ---- plane section queries (bm_planes.hip): the triangles each plane crosses and their cut segments ----
// What the query needs beyond TraceParams, as the kernel's second argument (TraceParams stays as it is): the
// hit-attribute table, since the sides are taken on the meshes' own vertices, and the segment records.
struct PlaneParams {
    const AttrMesh* meshes;   // num_meshes entries; slot[BM_VERTEX_DATA_POSITION]: the positions read
    const uint32_t* offsets;  // their tri_offset again, packed for the search
    uint32_t num_meshes;
    uint32_t pad;
    float4* segs;             // BM_PLANES_LIST: bm_segment records, two float4 each; may be null
};
// For each of p.q_n planes, two float4 (point, pad) (normal, pad) each in p.q_rays; set up as for
// launch_overlap_boxes, under the same names: p.q_out counts or bytes, p.q_ent the LIST offsets, p.q_counts the
// LIST ids (may be null when x.segs is not). count: into p.counters[0..3] (node records, triangle tests, the
// sum of the counts, the deepest stack held).
hipError_t launch_section_planes(const TraceParams& p, const PlaneParams& x, uint32_t mode, bool count, hipStream_t s);

// ---- instance transforms (bm_xform.hip): world-space copies of instanced meshes' positions and normals ----
// One row per instance entry of the scene, in scene order; uploaded as a byte image, followed by the rows'
// unit_first again, packed for the search.
constexpr uint32_t XFORM_UNIT = 256;  // vertices per work unit (one wave, four per lane)
struct XformRow {
    const float* src_pos;  // the mesh's own slots, 3 floats per vertex
    const float* src_nrm;
    float* dst_pos;        // the entry's 16-byte aligned regions of the scene's pools
    float* dst_nrm;
    uint32_t nv;           // vertices
    uint32_t unit_first;   // work units of the entries before this one
    float x[12];           // the transform, row-major 3x4
    float c[9];            // bm_xform_normal_matrix(x)
    uint32_t pad;
};  // 128 B
static_assert(sizeof(XformRow) == 128, "XformRow is uploaded as a byte image: no padding");
// One launch for all rows: num_units = the sum of ceil(nv / XFORM_UNIT); prefix[e] = rows[e].unit_first.
hipError_t launch_instance_xform(const XformRow* rows, const uint32_t* prefix, uint32_t num_entries,
                                 uint32_t num_units, hipStream_t s);

// ---- vertex normals (bm_normals.hip): a mesh's normal slot from its positions and indices ------------------
// offsets[nv + 1] and corners[num_indices]: the vertex -> corner table, the corner ids 3f + k stably sorted by
// their vertex (the host builds it, bm_api.cpp). Writes 3 * nv floats at nrm; nv = 0 launches nothing.
hipError_t launch_vertex_normals(const float* pos, const uint32_t* idx, const uint32_t* offsets,
                                 const uint32_t* corners, float* nrm, uint32_t nv, bool normalize, hipStream_t s);

// ---- reference mode (bm_kd.hip): the reference's kd-tree and march ---------------------------------
struct KdBuild {
    const MeshDesc* meshes;
    uint32_t num_meshes, n;
    float wmin, wmax;
    int leaf_depth;
    uint32_t* counts;   // n: leaves reached per triangle
    uint32_t* offsets;  // n: exclusive scan of counts
    uint32_t* keys;     // leaf path keys of the (key, triangle) pairs
    uint32_t* vals;
    uint32_t* cache;    // KD_LEAF_CACHE x n: the first leaves the count pass reached (slot i of g at i * n + g)
    // split descent (k_kd_top + k_kd_sub): split = 0 or >= leaf_depth walks each triangle in one lane
    int split = 0;
    uint2* queue = nullptr;      // queue_cap (triangle, path) items: the nodes reached at depth `split`
    uint32_t queue_cap = 0;
    uint32_t* qcount = nullptr;  // 2 words: queue length, overflow flag (a subtree walked on, not queued)
    // count pass: the 2,048-bit map of the top 11 path bits of the nodes reached at depth `split`, queued or
    // not (KD_TOPMAP_WORDS words, zeroed; only with split >= KD_TOP_BITS)
    // and the number of bits set (one word, zeroed) — the pair sort's ranked top digit (launch_sort_pairs)
    uint32_t* topmap = nullptr;
    uint32_t* topcount = nullptr;
    bool reuse_queue = false;    // emit: the count pass's queue is complete (flag read back 0)
    uint32_t* fill = nullptr;    // n: emit cursors
    uint32_t lq_cap = 0;         // LDS queue items per workgroup (0 or above the kernel's array: the array size)
    bool qcount_zeroed = false;  // qcount/overflow words already zero (launch_gather): the count pass skips its fill
    // emit pass: k_kd_sub also zero-fills these words (the pair sort's metadata: no fill launch before it);
    // *zeroed reports whether it ran
    uint32_t* zero_ptr = nullptr;
    uint32_t zero_words = 0;
    bool* zeroed = nullptr;
    const Tuning* tune = nullptr;  // BM_PARAM_KD_GRID / KD_PAIR / KD_TB
};
// The pair sort's ranked top digit: path bits of depths 0-10. The count pass can mark them only from nodes
// queued at a hand-off depth of at least this many levels, so a shallower split gets no map (kd_build).
constexpr uint32_t KD_TOP_BITS = 11;
// Depth at which the reference-mode build hands subtrees to other lanes (BM_PARAM_KD_SPLIT overrides; 0 = off)
int kd_split_depth(int leaf_depth, const Tuning& t);
constexpr uint32_t KD_LEAF_CACHE = 8;  // a triangle reaching at most this many leaves is not descended twice
struct KdMarch {
    const uint32_t *leaf_key, *leaf_start, *leaf_count, *faces, *lch, *rch, *first, *last;
    uint32_t num_leaves;
    int leaf_depth;
    float wmin, wmax;
    const uint4* nodes;   // march records (launch_kd_records): 2 x uint4 per internal node (num_leaves - 1)
    const uint4* leaves;  // 2 x uint4 per leaf
    const uint32_t* node_key;  // key of each internal node's first leaf
    const float4* ftris;  // 3 per sorted (leaf, face) pair: the face's triangle record (launch_kd_leaves)
    const uint32_t* ubox = nullptr;  // union of the leaf cells, 6 bound-slot images (launch_kd_records); null: no cull
    int march_variant = 3;  // 3: child-box steps (cnodes); 2: wave-cooperative leaves; 1 / 0: lane-per-ray leaves
    const uint32_t* num_leaves_dev = nullptr;  // build: the leaf count on the device (num_leaves bounds the grid)
    const uint4* cnodes = nullptr;  // child-box records: 4 x uint4 per internal node (launch_kd_records); null: none
    bool no_grid = false;  // BM_PARAM_KD_GRID 0: node boxes by the halving recurrence, never the closed form
};
// Build the march's node and leaf records from the Karras arrays of a reference-mode build.
// cnodes (optional): the child-box records the product march steps with (4 x uint4 per internal node).
// ubox (optional): the union of the leaf cells' boxes into ubox[6] as bound-slot images (bkey_lo of
// the minima, bkey of the maxima; ubox zero-filled by launch_kd_leaves first).
// The leaves' pair counts too (into k.leaf_count, from k.leaf_start and the pair count m). post_host
// (optional): launch_post's readback of *k.num_leaves_dev with sequence post_seq, done by the kernel itself.
hipError_t launch_kd_records(const KdMarch& k, uint32_t m, uint4* nodes, uint4* leaves, uint32_t* node_key,
                             hipStream_t s, uint4* cnodes = nullptr, uint32_t* ubox = nullptr,
                             uint32_t* post_host = nullptr, uint32_t post_seq = 0);
int kd_leaf_depth(float wmin, float wmax);
uint32_t scan_sums_words(uint32_t n);
// Exclusive scan of n u32 in one launch (decoupled look-back). sums: scan_sums_words(n) words of
// scratch, zero-filled once when allocated, then reused with a new epoch (1..2^20-1, != the last call's)
// per call; in/out 16-byte aligned. *grand_total = the u32 total and, with total64, *total64 = the exact
// 64-bit total (the pair-count guard of the reference-mode builds). run_keys (in unused): the scan of
// the run-start flags of n sorted keys (1 where key i differs from key i - 1), computed on the fly.
hipError_t launch_exclusive_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* sums,
                                 uint32_t* grand_total, hipStream_t s, unsigned long long* total64, uint32_t epoch,
                                 const uint32_t* run_keys = nullptr);
hipError_t launch_kd_count(const KdBuild& k, hipStream_t s);
constexpr uint64_t MAX_PAIRS = 0x7FFFFFFFull;  // (key, triangle) pairs a reference-mode build accepts
hipError_t launch_kd_emit(const KdBuild& k, hipStream_t s);
// leaf_count null: no count pass here (launch_kd_records computes the counts); flags null: run starts
// from the keys; ubox: zero-filled (the union words of launch_kd_records); ftris: the march's face
// records gathered in pair order too (faces[i]'s tri_orig record)
hipError_t launch_kd_leaves(const uint32_t* keys, uint32_t m, const uint32_t* flags, const uint32_t* leaf_of,
                            uint32_t* leaf_key, uint32_t* leaf_start, uint32_t* leaf_count, uint32_t nl,
                            hipStream_t s, const uint32_t* nl_dev = nullptr, uint32_t* ubox = nullptr,
                            const uint32_t* faces = nullptr, const float4* tri_orig = nullptr, float4* ftris = nullptr);
// Leaf-side kernels given the device leaf count (nl_dev) treat their host `nl` as the buffers' capacity:
// a device count above it (a build past BM_PARAM_KD_MAX_LEAVES) makes them write nothing, and the host
// reports the error when it reads the count (kd_leaves_ready).
constexpr uint32_t KD_MAX_LEAVES = 1u << 25;  // k_kd_records packs child indices below 2^25 with the split depth
// count: node records visited, face tests, hits into p.counters; p.diag: per-wave timeline (8x8 waves)
hipError_t launch_kd_march(const TraceParams& p, const KdMarch& k, bool count, hipStream_t s);

// ---- reference mode, hashed grid (bm_kd.hip): the reference's alternative accelerator (Hash.cu) ----
constexpr uint32_t HG_NUM_BUCKETS = 65536;     // MAX_HASH_ELEMENTS, BuildTree.cuh:21
constexpr uint32_t HG_MAX_CELLS = 1u << 20;    // cells per triangle AABB a build accepts
struct HashBuild {
    const MeshDesc* meshes;
    uint32_t num_meshes, n;
    uint32_t* counts;     // n: accepted cells per triangle
    uint32_t* offsets;    // n: exclusive scan of counts
    uint32_t* keys;       // bucket of each (cell, triangle) pair
    uint32_t* vals;       // its triangle id
    uint32_t* too_large;  // set when some triangle's AABB spans more than HG_MAX_CELLS cells
};
hipError_t launch_hash_count(const HashBuild& h, hipStream_t s);
hipError_t launch_hash_emit(const HashBuild& h, hipStream_t s);
hipError_t launch_hash_ranges(const uint32_t* keys, uint32_t m, uint32_t* bstart, uint32_t* bend, hipStream_t s);
hipError_t launch_hash_march(const TraceParams& p, const uint32_t* bstart, const uint32_t* bend,
                             const uint32_t* faces, hipStream_t s);
hipError_t launch_clear(uint32_t* buf, uint32_t pitch_u32, uint32_t width, uint32_t height, uint32_t value,
                        hipStream_t s);

// ---- multi-GPU exchange (bm_gather.hip) -------------------------------------------------------------
constexpr uint32_t PLANE_PACKED = 1, PLANE_TRI_ID = 2, PLANE_T = 4, PLANE_NZ = 8, PLANE_SHADOW = 16;
constexpr uint32_t MAX_BAND_SOURCES = 8;
struct BandPlanes {  // one device's band buffer: compact rows, row stride = frame width
    const uint32_t* packed;
    const uint32_t* tri;
    const float* t;
    const float* nz;        // may be null
    const uint8_t* shadow;  // may be null
    uint32_t band_first;    // the device's index: it holds bands b with b % band_step == band_first
    uint32_t rows;          // compact rows present
};
struct FramePlanes {  // the root render target
    uint32_t* packed;
    uint32_t pitch_u32;
    uint32_t* tri;
    float* t;
    float* nz;
    uint8_t* shadow;
    uint32_t width, height;
};
// Copy band rows of nsrc sources into their frame rows (the planes in `planes`). The launch runs on
// `s`'s device; source and destination may be on other devices when peer access is enabled.
hipError_t launch_band_scatter(const BandPlanes* src, uint32_t nsrc, const FramePlanes& dst, uint32_t band_h,
                               uint32_t band_step, uint32_t planes, hipStream_t s);

// Multi-GPU exchange by triangle id: rebuild packed, t and |n.z| of a full frame (p.width x p.height,
// p.tri_id filled) on the root from the ids, the camera tables and the scene's original-order
// triangle records (bm_trace.hip).
hipError_t launch_reshade(const TraceParams& p, const float4* tri_orig, hipStream_t s);
// Self-test of the trace's scalar primitives on n records (bm_debug_primitives; layouts: orc_pin_ops).
hipError_t launch_pin_ops(uint32_t n, const float* in, float* out, hipStream_t s);

// ---- RCCL, loaded on first use (bm_rccl.cpp): librccl.so.1, the same library torch uses ---------------
struct Rccl;
// nullptr (and *why set) when librccl.so.1 or one of its entry points cannot be loaded.
const Rccl* rccl_load(const char** why);
int rccl_unique_id(const Rccl* r, uint8_t* id128);
int rccl_init_rank(const Rccl* r, void** comm, int size, const uint8_t* id128, int rank);
int rccl_init_all(const Rccl* r, void** comms, int n, const int* devices);
void rccl_destroy(const Rccl* r, void* comm);
int rccl_group_start(const Rccl* r);
int rccl_group_end(const Rccl* r);
// bytes as ncclUint8 (0 = ncclSuccess)
int rccl_send(const Rccl* r, const void* buf, size_t bytes, int peer, void* comm, hipStream_t s);
int rccl_recv(const Rccl* r, void* buf, size_t bytes, int peer, void* comm, hipStream_t s);
const char* rccl_error_string(const Rccl* r, int code);

}  // namespace bm
