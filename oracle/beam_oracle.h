/*
 * beam_oracle.h — CPU oracle for the Beam primary-ray hot path.
 *
 * TEST INFRASTRUCTURE ONLY. Nothing in the product (raytracercuda_amd/, include/) may include,
 * link or call this. It is used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg, and there only as the checker / the timed CPU baseline, never as the thing shipped.
 *
 * Two restatements live here (plain C, IEEE f32, no FMA contraction, see oracle/Makefile):
 *
 *   1. Reference semantics ("kd"): the reference's sparse spatial-median kd-tree over the fixed
 *      world box [-30,30]^3 (Raytracer/BuildTree.cu:154-256, Raytracer/BoxTriangle.cuh:57-222)
 *      and its per-pixel march with first-hit-leaf early-out (BuildTree.cu:367-499). This is
 *      what the reference framebuffer contains. Pinned against the known answers recorded in
 *      SURVEY.md §8(c) (hit count + sum of packed u32) — see tests/test_oracle_golden.py.
 *
 *   2. Closest-hit LBVH ("bvh"): the exact algorithm the HIP path runs (Morton codes, stable
 *      LSD radix sort, Karras 2012 radix-tree emit, bottom-up refit, leaf collapse, near-first
 *      stack traversal), using the reference's Möller-Trumbore and shading arithmetic
 *      (Raytracer/CudaComon.cuh:117-155, 243-266) in glm 0.9.9.0 operation order. It is the
 *      parity reference for the GPU output (bit-exact node records, tri ids, packed colour, t)
 *      and the scalar CPU baseline timed by bench.py.
 *
 * Parity status: the reference itself is NOT buildable in this image without writing a stand-in
 * for <cuda_runtime.h> (CudaComon.cuh:7, SharedTypes.h:5), which the task rules forbid; the kd
 * restatement is therefore pinned by the SURVEY §8(c) known answers (produced by the survey's
 * probe of the reference CPU-emulation path), not by a build made here. The scalar primitives both
 * restatements share (orient*ray, 1/dir, bmTriIntersect, interpolate+normalize+pack) are pinned bit
 * for bit against the reference's vendored glm 0.9.9.0 compiled here (oracle/glm_pin.cpp,
 * tests/test_oracle_glm_pin.py). See DESIGN.md §3.
 */
#ifndef BEAM_ORACLE_H
#define BEAM_ORACLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One mesh: positions (slot 0, 3 floats/vertex), normals (slot 1, 3 floats/vertex, may be NULL),
 * u32 triangle-list indices. Mirrors StaticMeshData (Raytracer/SharedTypes.h:10-18). */
typedef struct orc_mesh {
    const float*    pos;
    const float*    nrm;
    const uint32_t* idx;
    uint32_t        num_verts;
    uint32_t        num_idx;
} orc_mesh;

/* The scalar primitives (orient*ray, 1/dir, bmTriIntersect, interpolate+normalize+pack) on a batch
 * of records, for the glm pin (layout in beam_oracle.c; tests/test_oracle_glm_pin.py). */
void orc_pin_ops(uint32_t n, const float* in, float* out);

/* Camera::setInitialRays (Raytracer/Camera.cpp:43-72): out[w*h*3] unit directions.
 * Returns 0 (ERROR_ALL_FINE) or 2 (ERROR_INVALID_PARAMETER). */
int32_t orc_camera_rays(uint32_t w, uint32_t h, float left, float right, float top, float bottom,
                        float zoom, float* out);

/* ---- 1. reference semantics: kd-tree + march ---------------------------------------------- */
typedef struct orc_kd orc_kd;
orc_kd* orc_kd_build(const orc_mesh* meshes, uint32_t num_meshes, float wmin, float wmax);
/* stats[0]=nodes [1]=leaves [2]=face refs stored [3]=dropped (leaf cap 256) [4]=max leaf count
 * [5]=max leaf depth */
void    orc_kd_stats(const orc_kd* kd, uint64_t stats[8]);
/* The leaves that hold faces (count > 0, all at the tree's one leaf depth), in ascending key order.
 * keys[i]: the root-to-leaf path, depth 0 in the highest of the leaf-depth bits, right = 1 (the low 32
 * bits of it for a tree deeper than 32); counts[i]: faces inserted (counts past the 256 cap);
 * faces: the stored ids of leaf 0, then of leaf 1, ...: the first min(count, 256) of each in insertion
 * order (stats[2] entries in all); *depth: the leaf depth (0 without leaves). Any pointer may be NULL.
 * Returns the number of leaves. Not stats[1], which also counts childless nodes above the leaf depth. */
uint32_t orc_kd_leaves(const orc_kd* kd, uint32_t* keys, uint32_t* counts, uint32_t* faces, uint32_t* depth);
void    orc_kd_free(orc_kd* kd);
/* March pixels [begin,end) of a ray table. Any output pointer may be NULL. Miss: packed=0xFF00,
 * tri=0xFFFFFFFF, t=+inf. Returns 0 or 4 (a mesh without normals, where the reference would
 * dereference NULL at BuildTree.cu:489). */
int32_t orc_kd_march(const orc_kd* kd, const float* rays, uint32_t begin, uint32_t end,
                     const float eye[3], const float orient_colmajor[9],
                     uint32_t* packed, uint32_t* tri_id, float* t);

/* The march's work over pixels [begin,end): counts[0] node pops (box tests: the reference's
 * bmStackNode pops), counts[1] leaves with faces entered, counts[2] face tests. */
int32_t orc_kd_march_counts(const orc_kd* kd, const float* rays, uint32_t begin, uint32_t end,
                            const float eye[3], const float orient_colmajor[9], uint64_t counts[3]);

/* ---- 1b. reference semantics: hashed uniform grid (Hash.cu, insert loop fixed) --------------- */
typedef struct orc_hash orc_hash;
/* NULL when a triangle's AABB spans more than 2^20 cells of 0.03 */
orc_hash* orc_hash_build(const orc_mesh* meshes, uint32_t num_meshes);
void      orc_hash_free(orc_hash* h);
/* stats[0]=(cell, face) pairs [1]=non-empty buckets [2]=max bucket count [3]=dropped (cap 256) */
void      orc_hash_stats(const orc_hash* h, uint64_t stats[4]);
/* bucket b holds faces[start[b] .. start[b+1]) (global triangle ids, insertion order) */
const uint32_t* orc_hash_buckets(const orc_hash* h, const uint32_t** faces);
/* March pixels [begin,end) of a ray table; outputs and return codes as orc_kd_march. */
int32_t   orc_hash_march(const orc_hash* h, const float* rays, uint32_t begin, uint32_t end,
                         const float eye[3], const float orient_colmajor[9],
                         uint32_t* packed, uint32_t* tri_id, float* t);

/* ---- 2. closest-hit LBVH (the GPU algorithm) ------------------------------------------------ */
typedef struct orc_bvh orc_bvh;
orc_bvh* orc_bvh_build(const orc_mesh* meshes, uint32_t num_meshes, uint32_t leaf_size);
/* width 4: the BVH4 layout (every other level of the binary tree collapsed, 128-B records with
 * SoA child boxes); width 2 is orc_bvh_build. */
orc_bvh* orc_bvh_build_ex(const orc_mesh* meshes, uint32_t num_meshes, uint32_t leaf_size,
                          uint32_t width);
uint32_t orc_bvh_record_words(const orc_bvh* b);  /* 16 (BVH2) or 32 (BVH4) u32 per record */
/* Refit to new vertex data of the same meshes (same triangle count; topology of the last build
 * kept): returns 0, or 2 when the triangle count differs. */
int32_t  orc_bvh_refit(orc_bvh* b, const orc_mesh* meshes, uint32_t num_meshes);
/* Experiment hook for tools/: pack and traverse a caller-given binary tree (see beam_oracle.c). */
orc_bvh* orc_bvh_build_tree(const orc_mesh* meshes, uint32_t num_meshes, uint32_t leaf_size,
                            uint32_t width, const uint32_t* perm, const uint32_t* lch,
                            const uint32_t* rch);
void     orc_bvh_free(orc_bvh* b);
uint32_t orc_bvh_num_tris(const orc_bvh* b);
uint32_t orc_bvh_num_records(const orc_bvh* b);   /* = max(n-1, 1) (slot per Karras internal node) */
/* Export for structural parity: records[num_records*record_words] (u32 bit patterns), tris[n*12] (u32 bit
 * patterns, sorted order), keys[n] sorted Morton keys, perm[n] sorted->original global id. Any
 * pointer may be NULL. */
void     orc_bvh_export(const orc_bvh* b, uint32_t* records, uint32_t* tris, uint32_t* keys,
                        uint32_t* perm);
/* Closest hit with t > 0, ties on equal t to the lowest global triangle id. counters (may be
 * NULL): [0] node records fetched, [1] triangle tests, [2] hits. */
int32_t  orc_bvh_trace(const orc_bvh* b, const float* rays, uint32_t begin, uint32_t end,
                       const float eye[3], const float orient_colmajor[9],
                       uint32_t* packed, uint32_t* tri_id, float* t, uint64_t counters[3]);

/* Record per-ray work (2 u32 per pixel index: node records, triangle tests) in later
 * orc_bvh_trace calls; NULL turns it off. */
void     orc_set_ray_stats(uint32_t* per_ray);
/* Deepest traversal stack seen since the last orc_set_ray_stats call. */
int32_t  orc_max_stack(void);
/* Record each ray's deepest traversal stack (1 u32 per pixel index: the largest number of entries its
 * stack held after a node step's pushes) in later orc_bvh_trace and orc_bvh_shadow calls of the calling
 * thread; NULL turns it off. orc_bvh_shadow records the shadow ray's own depth, 0 where none is cast.
 * The GPU kernels push in the same order (the traversal counters match), so this is the depth their
 * stacks must reach: entries past a kernel's LDS depth live in its global overflow area. */
void     orc_set_ray_depth(uint32_t* per_ray);

/* One shadow ray per primary hit (build-defined, the reference has none):
 * origin = eye + dir * (t * 0.9999f), direction = light - origin (unnormalised); the pixel is
 * shadowed (1) when any triangle's Möller-Trumbore t_s satisfies 0 < t_s < 1, else 0; a primary
 * miss gives 0. tri_id/tprim are the primary frame (indexed like rays). Any-hit traversal in the
 * GPU kernel's order, so counters ([0] node records, [1] triangle tests, [2] shadowed pixels)
 * match the GPU's COUNT build. */
int32_t  orc_bvh_shadow(const orc_bvh* b, const float* rays, uint32_t begin, uint32_t end,
                        const float eye[3], const float orient_colmajor[9], const float light[3],
                        const uint32_t* tri_id, const float* tprim, uint8_t* shadow,
                        uint64_t counters[3]);
/* Exhaustive any-hit version of orc_bvh_shadow (same acceptance rule) over every triangle. */
int32_t  orc_brute_shadow(const orc_mesh* meshes, uint32_t num_meshes, const float* rays,
                          uint32_t begin, uint32_t end, const float eye[3],
                          const float orient_colmajor[9], const float light[3],
                          const uint32_t* tri_id, const float* tprim, uint8_t* shadow);

/* Exhaustive closest hit (same acceptance rule as orc_bvh_trace) over every triangle. */
int32_t  orc_brute_trace(const orc_mesh* meshes, uint32_t num_meshes, const float* rays,
                         uint32_t begin, uint32_t end, const float eye[3],
                         const float orient_colmajor[9], uint32_t* packed, uint32_t* tri_id,
                         float* t);

/* OBJ reader used only to produce tests/golden mesh fixtures: mesh-per-usemtl in file order,
 * corners unshared (position v[vi], normal vn[ni]); strtof parsing. share=1 shares vertices when
 * every corner has vi == ni; share=2 shares them and takes normals by the POSITION index vn[vi]
 * (the survey loader's convention for suzanne). Returns number of meshes
 * or <0. Buffers are malloc'd and released by orc_obj_free. */
typedef struct orc_obj {
    uint32_t num_meshes;
    float*    pos[16];
    float*    nrm[16];
    uint32_t* idx[16];
    uint32_t  num_verts[16];
    uint32_t  num_idx[16];
} orc_obj;
int32_t orc_obj_load(const char* path, int32_t share_vertices, orc_obj* out);
void    orc_obj_free(orc_obj* o);

#ifdef __cplusplus
}
#endif
#endif
