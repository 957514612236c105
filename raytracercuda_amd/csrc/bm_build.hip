// bm_build.hip — LBVH acceleration-structure build for gfx950 (replaces the reference's
// sparse kd-tree insert, Raytracer/BuildTree.cu:95-362, and its SAT test, BoxTriangle.cuh).
//
// Pipeline (one HIP stream, no host round trips; 1.1M triangles in 0.29 ms on one MI355X):
//   memset          the gather's bounds replicas (the rest of the metadata block: k_gather)
//   k_gather        mesh table -> per-triangle (v0,e1,e2,id) records, corner normals, AABBs (stores
//                   staged through LDS); block-reduced scene/centroid bounds via ordered-int atomics
//                   into 64 replicas (folded by their consumers: k_morton, k_span_chunk)
//   k_morton        30-bit Morton key of each AABB centre, value = global triangle id; the digit
//                   histograms of all three sort passes
//   k_onesweep_wide x3  stable LSD radix sort, 10-bit digits, one kernel per pass: 1024-thread tiles
//                   (one digit per thread), decoupled look-back over a 32-word window, wave64 ballot
//                   ranking, the tile staged in LDS in digit order before the scatter
//   k_span_chunk    one launch (k_tree_chunk alone up to 512 triangles), two kinds of workgroup:
//     span          (n > 512) the radix-tree nodes whose leaf range crosses a 512-leaf chunk edge:
//                   O(1) test per index, Karras's searches 64-ary per wave; a bitmap of them
//     chunk         per 512-leaf chunk, in LDS: the chunk-local nodes grown bottom-up (Apetrei's
//                   rule, Karras's indices) with their boxes, the triangle records in leaf order,
//                   prefix/suffix box unions at maximal-subtree ends, and (BVH4) the 128-B record of
//                   every chunk-local node above the leaf size
//   k_chunk_table   sparse table over the chunk unions (boxes of chunk-spanning ranges in O(1))
//   k_pack4_span / k_pack   BVH4 records of the spanning nodes (or all BVH2 records)
// Refit (same topology, new vertices): memset, k_gather, then k_span_chunk .. k_pack4_span as above.
// Every stored value is a deterministic function of the input (no atomics decide a value), so
// the result is bit-identical to oracle/beam_oracle.c's orc_bvh_build, which tests check.
#include <climits>

#include "bm_internal.h"

namespace bm {
namespace {

#include "bm_bdiag.h"

constexpr int BLOCK = 256;
constexpr int SORT_ITEMS = 16;  // histogram kernels; the one-sweep tile is chosen per n (onesweep_items)
constexpr int SORT_TILE = BLOCK * SORT_ITEMS;
inline uint32_t blocks_for(uint32_t n, uint32_t per) { return (n + per - 1) / per; }
constexpr uint32_t REFIT_CHUNK_LOG2 = 9;  // 512-leaf chunks: measured 2-4 % faster builds than 1024 up to 1.1M tris (256: slower at 1.1M)
constexpr uint32_t REFIT_CHUNK = 1u << REFIT_CHUNK_LOG2;

// Wave64 reductions on the VALU: DPP within rows of 16 (quad_perm [1,0,3,2], [2,3,0,1], row_ror 4
// and 8), then the four row results via readlane. Every lane of the wave must be active.
template <bool MAX>
__device__ __forceinline__ int wave_reduce(int v) {
    auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, false));
    return op(op(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
              op(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_min(int v) { return wave_reduce<false>(v); }
__device__ __forceinline__ int wave_max(int v) { return wave_reduce<true>(v); }

// ---- build metadata block (one zero fill per build) ----------------------------------------------
//   [0, BOUNDS_SLOTS)               scene bounds (bm_common.h)
//   [META_GATHER_REPLICAS, +GATHER_REPLICAS * GATHER_REPLICA_STRIDE)  k_gather's bounds replicas
//   [META_COUNTERS, +4)             per-pass tile tickets of the one-sweep sort
//   [META_GHIST, +3*RADIX)          global digit histograms of all passes
//   [META_LOOKBACK, +3*nb*RADIX)    per-pass, per-tile, per-digit look-back words
constexpr int RADIX_BITS = 10;  // stable LSD radix sort: 3 passes of 10-bit digits over 30-bit keys
constexpr uint32_t RADIX = 1u << RADIX_BITS;
constexpr int RADIX_PASSES = 3;
constexpr uint32_t GATHER_REPLICAS = 64;
constexpr uint32_t GATHER_REPLICA_STRIDE = 32;  // 128 B apart
constexpr uint32_t META_GATHER_REPLICAS = 32;
constexpr uint32_t META_COUNTERS = META_GATHER_REPLICAS + GATHER_REPLICAS * GATHER_REPLICA_STRIDE;
constexpr uint32_t META_GATHER_CLEAR = META_COUNTERS;  // what a gather-only pass (refit, kd) zero-fills
constexpr uint32_t META_SORT_SKEW = META_COUNTERS + 3;  // buckets k_bucket_sort sorted through global memory
constexpr uint32_t META_GHIST = META_COUNTERS + 4;
constexpr uint32_t META_LOOKBACK = META_GHIST + RADIX_PASSES * RADIX;

// Triangles -> original-order records (v0, e1, e2 + id), corner normals, AABBs and/or AABB centres
// (each output optional), and the scene bounds of the AABBs and of their centres.
// Also zero-fills meta words [clear_begin, clear_end) — a build's: the sort's counters, histograms and
// look-back words, first used by k_morton, and the finish counters; a refit's: the finish counters —
// so that only the gather's own words need a memset.
__global__ __launch_bounds__(BLOCK) void k_gather(const MeshDesc* __restrict__ meshes, uint32_t nm, uint32_t n,
                                                  float4* __restrict__ tri, float* __restrict__ nrm,
                                                  float* __restrict__ aabb, float* __restrict__ cen,
                                                  uint32_t* __restrict__ bounds,
                                                  uint32_t clear_begin, uint32_t clear_end, int with_bounds,
                                                  int with_tri, int with_nrm) {
    BDIAG(0);
    for (uint32_t q = clear_begin + blockIdx.x * BLOCK + threadIdx.x; q < clear_end; q += gridDim.x * BLOCK)
        bounds[q] = 0u;
    // the block's records, corner normals and boxes are staged in LDS and stored as whole float4
    // runs (a lane's own 48-, 36- and 24-byte records would be strided, partial-line stores)
    __shared__ float4 s_tri[3 * BLOCK];
    __shared__ float s_nrm[9 * BLOCK];
    __shared__ float s_box[6 * BLOCK];
    __shared__ float s_cen[3 * BLOCK];
    const uint32_t g0 = blockIdx.x * BLOCK, g = g0 + threadIdx.x;
    int lo[6], hi[6];  // ordered ints: [0..2] aabb, [3..5] centre
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        lo[c] = INT_MAX;
        hi[c] = INT_MIN;
    }
    if (g < n) {
        uint32_t a = 0, b = nm;
        while (b - a > 1) {
            uint32_t mid = (a + b) >> 1;
            if (meshes[mid].tri_offset <= g) a = mid;
            else b = mid;
        }
        const MeshDesc md = meshes[a];
        const uint32_t f = g - md.tri_offset;
        const uint32_t i0 = md.idx[3 * f], i1 = md.idx[3 * f + 1], i2 = md.idx[3 * f + 2];
        const vec3f p0 = v3(md.pos[3 * i0], md.pos[3 * i0 + 1], md.pos[3 * i0 + 2]);
        const vec3f p1 = v3(md.pos[3 * i1], md.pos[3 * i1 + 1], md.pos[3 * i1 + 2]);
        const vec3f p2 = v3(md.pos[3 * i2], md.pos[3 * i2 + 1], md.pos[3 * i2 + 2]);
        if (with_tri) {
            const vec3f e1 = sub(p1, p0), e2 = sub(p2, p0);
            s_tri[3 * threadIdx.x + 0] = make_float4(p0.x, p0.y, p0.z, u2f(g));
            s_tri[3 * threadIdx.x + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
            s_tri[3 * threadIdx.x + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
        }
        if (with_nrm) {
            const uint32_t iv[3] = {i0, i1, i2};
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) s_nrm[9 * threadIdx.x + 3 * k + c] = md.nrm[3 * iv[k] + c];
        }
        const float pa[3] = {p0.x, p0.y, p0.z}, pb[3] = {p1.x, p1.y, p1.z}, pc[3] = {p2.x, p2.y, p2.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float mn = omin(omin(pa[c], pb[c]), pc[c]);
            const float mx = omax(omax(pa[c], pb[c]), pc[c]);
            const float ce = (mn + mx) * 0.5f;
            s_box[6 * threadIdx.x + c] = mn;
            s_box[6 * threadIdx.x + 3 + c] = mx;
            s_cen[3 * threadIdx.x + c] = ce;
            lo[c] = ord(mn);
            hi[c] = ord(mx);
            lo[3 + c] = ord(ce);
            hi[3 + c] = ord(ce);
        }
    }
    __shared__ int s_lo[BLOCK / 64][6], s_hi[BLOCK / 64][6];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int a = wave_min(lo[c]), b = wave_max(hi[c]);
        if (lane == 0) {
            s_lo[w][c] = a;
            s_hi[w][c] = b;
        }
    }
    __syncthreads();
    const uint32_t cnt = min(n - g0, (uint32_t)BLOCK);
    if (cnt == BLOCK) {
        if (with_tri)
            for (uint32_t q = threadIdx.x; q < 3 * BLOCK; q += BLOCK) tri[3 * (size_t)g0 + q] = s_tri[q];
        if (with_nrm) {
            float4* nd = reinterpret_cast<float4*>(nrm + 9 * (size_t)g0);
            const float4* ns = reinterpret_cast<const float4*>(s_nrm);
            for (uint32_t q = threadIdx.x; q < 9 * BLOCK / 4; q += BLOCK) nd[q] = ns[q];
        }
        if (aabb) {
            float4* bd = reinterpret_cast<float4*>(aabb + 6 * (size_t)g0);
            const float4* bs = reinterpret_cast<const float4*>(s_box);
            for (uint32_t q = threadIdx.x; q < 6 * BLOCK / 4; q += BLOCK) bd[q] = bs[q];
        }
        if (cen) {
            float4* cd = reinterpret_cast<float4*>(cen + 3 * (size_t)g0);
            const float4* cs = reinterpret_cast<const float4*>(s_cen);
            for (uint32_t q = threadIdx.x; q < 3 * BLOCK / 4; q += BLOCK) cd[q] = cs[q];
        }
    } else {
        if (with_tri)
            for (uint32_t q = threadIdx.x; q < 3 * cnt; q += BLOCK) tri[3 * (size_t)g0 + q] = s_tri[q];
        if (with_nrm)
            for (uint32_t q = threadIdx.x; q < 9 * cnt; q += BLOCK) nrm[9 * (size_t)g0 + q] = s_nrm[q];
        if (aabb)
            for (uint32_t q = threadIdx.x; q < 6 * cnt; q += BLOCK) aabb[6 * (size_t)g0 + q] = s_box[q];
        if (cen)
            for (uint32_t q = threadIdx.x; q < 3 * cnt; q += BLOCK) cen[3 * (size_t)g0 + q] = s_cen[q];
    }
    // block bounds -> replica (block % GATHER_REPLICAS) of the twelve slots, each replica on its own
    // 128-B line (fold_slot reduces them). Device atomics on one address serialise (~15 ns each),
    // so thousands of blocks updating the same twelve words would cost tens of microseconds.
    if (threadIdx.x < 6 && with_bounds) {
        const int c = threadIdx.x;
        int a = s_lo[0][c], b = s_hi[0][c];
        for (int q = 1; q < BLOCK / 64; ++q) {
            a = min(a, s_lo[q][c]);
            b = max(b, s_hi[q][c]);
        }
        // slots: aabb min 0..2, aabb max 3..5, centre min 6..8, centre max 9..11
        const int slot_lo = c < 3 ? c : 6 + (c - 3);
        const int slot_hi = c < 3 ? 3 + c : 9 + (c - 3);
        // ordered ints -> order-preserving u32; min slots complemented (see BOUNDS_SLOTS)
        uint32_t* rep = bounds + META_GATHER_REPLICAS + GATHER_REPLICA_STRIDE * (blockIdx.x % GATHER_REPLICAS);
        atomicMax(&rep[slot_lo], ~((uint32_t)a ^ 0x80000000u));
        atomicMax(&rep[slot_hi], (uint32_t)b ^ 0x80000000u);
    }
}

// ---- a triangle straight from its mesh (k_gather's operations, shared by the mesh-direct readers) -----
// Global triangle g -> its mesh (binary search over the mesh table's first ids) -> its three corners.
__device__ __forceinline__ void tri_from_mesh(const MeshDesc* __restrict__ meshes, uint32_t nm, uint32_t g,
                                              vec3f& p0, vec3f& p1, vec3f& p2) {
    uint32_t a = 0, b = nm;
    while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (meshes[mid].tri_offset <= g) a = mid;
        else b = mid;
    }
    const MeshDesc md = meshes[a];
    const uint32_t f = g - md.tri_offset;
    const uint32_t i0 = md.idx[3 * f], i1 = md.idx[3 * f + 1], i2 = md.idx[3 * f + 2];
    p0 = v3(md.pos[3 * i0], md.pos[3 * i0 + 1], md.pos[3 * i0 + 2]);
    p1 = v3(md.pos[3 * i1], md.pos[3 * i1 + 1], md.pos[3 * i1 + 2]);
    p2 = v3(md.pos[3 * i2], md.pos[3 * i2 + 1], md.pos[3 * i2 + 2]);
}
// its AABB as ordered ints (lo xyz, hi xyz): k_gather's omin/omax, so the same bits as aabb[]
__device__ __forceinline__ void tri_box_ord(const vec3f& p0, const vec3f& p1, const vec3f& p2, int32_t (&o)[6]) {
    const float pa[3] = {p0.x, p0.y, p0.z}, pb[3] = {p1.x, p1.y, p1.z}, pc[3] = {p2.x, p2.y, p2.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = ord(omin(omin(pa[c], pb[c]), pc[c]));
        o[3 + c] = ord(omax(omax(pa[c], pb[c]), pc[c]));
    }
}
// its (v0 | id, e1, e2) record: k_gather's subtraction (bit-identical to bmTriIntersect's edges)
__device__ __forceinline__ void tri_record(const vec3f& p0, const vec3f& p1, const vec3f& p2, uint32_t g, float4& t0,
                                           float4& t1, float4& t2) {
    const vec3f e1 = sub(p1, p0), e2 = sub(p2, p0);
    t0 = make_float4(p0.x, p0.y, p0.z, u2f(g));
    t1 = make_float4(e1.x, e1.y, e1.z, 0.0f);
    t2 = make_float4(e2.x, e2.y, e2.z, 0.0f);
}

// Zero the gather's replica words (threads t of nthreads), after their last reader: the next LBVH
// build or refit of this buffer then needs no memset before k_gather (BuildBuffers::replicas_clean).
__device__ __forceinline__ void clear_replicas(uint32_t* __restrict__ bounds, uint32_t t, uint32_t nthreads) {
    for (uint32_t q = META_GATHER_REPLICAS + t; q < META_GATHER_CLEAR; q += nthreads) bounds[q] = 0u;
}

// Scene-bounds slot = max over the gather replicas. Folded where first needed: by k_morton (each
// block, into LDS), into bounds[0..11] by the first span workgroup of k_span_chunk, k_tree_chunk (one chunk) or
// k_pack_small for the record writers.
__device__ __forceinline__ uint32_t fold_slot(const uint32_t* __restrict__ bounds, int slot) {
    uint32_t acc = 0;
#pragma unroll 16
    for (uint32_t r = 0; r < GATHER_REPLICAS; ++r)
        acc = max(acc, bounds[META_GATHER_REPLICAS + GATHER_REPLICA_STRIDE * r + slot]);
    return acc;
}

// The same fold by one wave for six consecutive slots s0..s0+5: lane r reads replica r's six words
// (three 8-B loads from one 128-B line), then a wave maximum per slot. One memory round trip instead of
// 64 dependent-free loads per slot on six lanes; every lane of the wave must be active. Returns slot
// s0 + j in lane j (j < 6).
__device__ __forceinline__ uint32_t fold6_wave(const uint32_t* __restrict__ bounds, uint32_t s0) {
    static_assert(GATHER_REPLICAS == 64, "one replica per lane");
    const uint32_t lane = threadIdx.x & 63;
    const uint2* q = reinterpret_cast<const uint2*>(bounds + META_GATHER_REPLICAS + GATHER_REPLICA_STRIDE * lane + s0);
    const uint2 a = q[0], b = q[1], c = q[2];
    uint32_t v[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        uint32_t x = v[j];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, o));
        out = lane == (uint32_t)j ? x : out;
    }
    return out;
}

// Morton key of each AABB centre (value = global triangle id), plus the digit histograms of all
// three sort passes (a histogram does not depend on the order the keys are in).
// 1024-thread workgroups over SORT_TILE keys (4 per thread): sixteen waves hide the loads and the
// LDS histogram atomics of a tile where four could not.
constexpr int MORTON_BLOCK = 1024;
constexpr int MORTON_ITEMS = SORT_TILE / MORTON_BLOCK;
__global__ __launch_bounds__(MORTON_BLOCK) void k_morton(uint32_t n, const float* __restrict__ cen,
                                                         uint32_t* __restrict__ meta, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals) {
    BDIAG(1);
    __shared__ uint32_t h[RADIX_PASSES * RADIX];
    __shared__ uint32_t s_cb[6];  // centre bounds slots 6..11
    // all loads first (clamped index, no branches) and before the bounds fold's barrier, so the tile
    // pays one memory latency
    const uint32_t base = blockIdx.x * SORT_TILE;
    float ce[MORTON_ITEMS][3];
#pragma unroll
    for (int it = 0; it < MORTON_ITEMS; ++it) {
        const uint32_t g = min(base + it * MORTON_BLOCK + threadIdx.x, n - 1);
        // the AABB centres k_gather computed ((lo + hi) * 0.5f per axis)
        ce[it][0] = cen[3 * (size_t)g + 0];
        ce[it][1] = cen[3 * (size_t)g + 1];
        ce[it][2] = cen[3 * (size_t)g + 2];
    }
    for (uint32_t d = threadIdx.x; d < RADIX_PASSES * RADIX; d += MORTON_BLOCK) h[d] = 0;
    if (threadIdx.x < 64) {  // wave 0: centre bounds slots 6..11
        const uint32_t v = fold6_wave(meta, 6);
        if (threadIdx.x < 6) s_cb[threadIdx.x] = v;
    }
    __syncthreads();
    float cmin[3], scale[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        cmin[c] = bounds_lo(s_cb[c]);
        const float ext = bounds_hi(s_cb[3 + c]) - cmin[c];
        scale[c] = ext > 0.0f ? 1024.0f / ext : 0.0f;
    }
#pragma unroll
    for (int it = 0; it < MORTON_ITEMS; ++it) {
        const uint32_t g = base + it * MORTON_BLOCK + threadIdx.x;
        if (g >= n) break;
        uint32_t q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = quant10(ce[it][c], cmin[c], scale[c]);
        const uint32_t key = (expand_bits10(q[0]) << 2) | (expand_bits10(q[1]) << 1) | expand_bits10(q[2]);
        keys[g] = key;
        vals[g] = g;
#pragma unroll
        for (int p = 0; p < RADIX_PASSES; ++p) atomicAdd(&h[p * RADIX + ((key >> (p * RADIX_BITS)) & (RADIX - 1))], 1u);
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < RADIX_PASSES * RADIX; d += MORTON_BLOCK)
        if (h[d]) atomicAdd(&meta[META_GHIST + d], h[d]);
}

#include "bm_sort.h"

// ---- Karras 2012 radix tree ------------------------------------------------------------------
__device__ __forceinline__ int kdelta(const uint32_t* __restrict__ k, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const uint32_t a = k[i], b = k[j];
    if (a == b) return 32 + __clz((uint32_t)i ^ (uint32_t)j);
    return __clz(a ^ b);
}

// One internal node i of Karras's radix tree over n sorted keys (children, parents, covered range).
__device__ __forceinline__ void karras_node(int i, int n, const uint32_t* __restrict__ keys, uint32_t* __restrict__ lch,
                                            uint32_t* __restrict__ rch, uint32_t* __restrict__ first,
                                            uint32_t* __restrict__ last, uint32_t* __restrict__ parent_leaf,
                                            uint32_t* __restrict__ parent_int) {
    const int d = (kdelta(keys, n, i, i + 1) - kdelta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = kdelta(keys, n, i, i - d);
    int lmax = 2;
    while (kdelta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (kdelta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = kdelta(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (kdelta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = min(i, j), hi = max(i, j);
    if (lo == gamma) {
        lch[i] = (uint32_t)gamma | LEAF_BIT;
        parent_leaf[gamma] = (uint32_t)i;
    } else {
        lch[i] = (uint32_t)gamma;
        parent_int[gamma] = (uint32_t)i;
    }
    if (hi == gamma + 1) {
        rch[i] = (uint32_t)(gamma + 1) | LEAF_BIT;
        parent_leaf[gamma + 1] = (uint32_t)i;
    } else {
        rch[i] = (uint32_t)(gamma + 1);
        parent_int[gamma + 1] = (uint32_t)i;
    }
    first[i] = (uint32_t)lo;
    last[i] = (uint32_t)hi;
}

// Karras radix tree over the reference-mode leaf keys (16,742 on the bunny): every
// workgroup with nodes to emit first copies all keys into LDS, so the searches' ~2 log2(n) dependent key
// reads are LDS round trips instead of global ones (13 -> ~4 us on the bunny). More keys than the LDS
// holds: the global reads. n_dev: the key count on the device (n: the capacity).
constexpr uint32_t EMIT_LDS_KEYS = 32768, EMIT_LDS_BLOCK = 1024;
__global__ __launch_bounds__(EMIT_LDS_BLOCK) void k_emit_lds(int n, const uint32_t* __restrict__ keys,
                                                             uint32_t* __restrict__ lch, uint32_t* __restrict__ rch,
                                                             uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                             uint32_t* __restrict__ parent_leaf,
                                                             uint32_t* __restrict__ parent_int,
                                                             const uint32_t* __restrict__ n_dev) {
    __shared__ uint32_t sk[EMIT_LDS_KEYS];
    if (n_dev) n = *n_dev <= (uint32_t)n ? (int)*n_dev : 0;
    const int b0 = (int)(blockIdx.x * EMIT_LDS_BLOCK);
    if (b0 >= n - 1) return;  // the whole workgroup: no node here
    const int i = b0 + (int)threadIdx.x;
    if ((uint32_t)n <= EMIT_LDS_KEYS) {
        const int n4 = n >> 2;  // 16-B loads (the key buffer starts 16-B aligned), then the tail
        const uint4* k4 = reinterpret_cast<const uint4*>(keys);
        uint4* s4 = reinterpret_cast<uint4*>(sk);
#pragma unroll 4
        for (int q = (int)threadIdx.x; q < n4; q += (int)EMIT_LDS_BLOCK) s4[q] = k4[q];
        for (int q = 4 * n4 + (int)threadIdx.x; q < n; q += (int)EMIT_LDS_BLOCK) sk[q] = keys[q];
        __syncthreads();
        if (i < n - 1) karras_node(i, n, sk, lch, rch, first, last, parent_leaf, parent_int);
    } else if (i < n - 1) {
        karras_node(i, n, keys, lch, rch, first, last, parent_leaf, parent_int);
    }
}

__device__ __forceinline__ void child_box(uint32_t c, const uint32_t* __restrict__ perm, const float* __restrict__ aabb,
                                          const MeshDesc* __restrict__ meshes, uint32_t nm, const int32_t* ibox,
                                          float* lo, float* hi) {
    if ((c & LEAF_BIT) && !aabb) {  // mesh-direct builds keep no aabb[]: the leaf's box from its mesh
        vec3f p0, p1, p2;
        tri_from_mesh(meshes, nm, perm[c & ~LEAF_BIT], p0, p1, p2);
        int32_t o[6];
        tri_box_ord(p0, p1, p2, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = unord(o[a]);
            hi[a] = unord(o[3 + a]);
        }
    } else if (c & LEAF_BIT) {
        const float* p = aabb + 6 * (size_t)perm[c & ~LEAF_BIT];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = p[a];
            hi[a] = p[3 + a];
        }
    } else {
        const int32_t* p = ibox + 6 * (size_t)c;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = unord(p[a]);
            hi[a] = unord(p[3 + a]);
        }
    }
}

// Refit without any inter-workgroup hand-off inside a launch. A node's box is the union of the
// leaf boxes of its sorted range [first, last] (union = ordered-int min/max: exact and
// order-independent, so equal to the oracle's recursive refit bit for bit).
// k_tree_chunk: one workgroup per chunk of 512 sorted leaves. (1) In-chunk prefix and suffix unions
// of the leaf boxes (wave scans) -> pre[], suf[]. (2) Each thread climbs from its leaf through the
// nodes whose range lies inside the chunk (their indices do too: a Karras node's index is an end of
// its range), arrival counters and boxes in LDS, workgroup-scope acq_rel atomics -> ibox[].
// k_chunk_table: sparse table of whole-chunk unions (one workgroup).
// A node spanning chunks [cf, cl] then has box = suf[first] U table(cf+1..cl-1) U pre[last]:
// k_pack4_span / k_pack evaluate that directly; no chain of dependent steps remains.
// (A one-pass refit with agent-scope release/acquire per level cost ~0.26 ms at 70k triangles,
// a second single-workgroup climb over the spanning nodes ~50 us.)
// Boxes between the leaves and the node records (in-chunk node boxes, prefix/suffix unions, the
// chunk table) live as ordered-int images (ord): a union is then one v_min_i32/v_max_i32 per
// coordinate instead of two order conversions, a compare and a select, and unord at the record
// writer restores the floats bit for bit.
__device__ __forceinline__ void box_union(int32_t* r, const int32_t* a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[c] = min(r[c], a[c]);
        r[3 + c] = max(r[3 + c], a[3 + c]);
    }
}
__device__ __forceinline__ void box_identity(int32_t* r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[c] = INT_MAX;
        r[3 + c] = INT_MIN;
    }
}

// ---- radix tree + chunk refit in one pass ---------------------------------------------------
// Karras's tree is the binary radix tree of the sorted keys (position tiebreak), so it can also be
// grown bottom-up (Apetrei 2014): a node [l, r] is the LEFT child of its parent iff
// delta(r, r+1) > delta(l-1, l) (ties are impossible for distinct augmented keys), its parent's
// split is then r (else l-1), and its Karras index is the end of its range facing the split (a
// left child's index is its split side r, a right child's its l). k_tree_chunk grows every node
// whose range lies in one 512-leaf chunk that way with the chunk's keys and deltas in LDS (two
// arrivals per split, workgroup-scope atomics), computing its box on the way; the nodes whose range
// crosses a chunk edge ("spanning" nodes, about ten per chunk edge: 22k at 1.1M triangles) are
// found by Karras's searches, run 64-ary by one wave each (a dozen dependent loads where the binary
// searches of a per-node Karras kernel took up to ~60). The result is karras_node's tree, bit for bit.
constexpr unsigned long long SLOT_EMPTY = ~0ull, SLOT_DONE = ~0ull - 1;  // k_tree_chunk split words

__device__ __forceinline__ int kdelta_aug(uint32_t a, uint32_t b, uint32_t i, uint32_t j) {
    return a == b ? 32 + __clz(i ^ j) : __clz(a ^ b);
}

// Largest m in [lo, hi) with pred(m), for pred monotone (true, then false) and pred(lo) true;
// one round of 64 probes per 64-fold shrink. Wave-uniform arguments, every lane active.
template <class Pred>
__device__ __forceinline__ uint32_t wave_last_true(uint32_t lo, uint32_t hi, Pred pred) {
    const uint32_t lane = threadIdx.x & 63;
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + 63) >> 6;
        const uint32_t m = lo + step * (lane + 1);
        const unsigned long long mask = ballot(m < hi && pred(m));
        if (mask) lo += step * (uint32_t)(64 - __clzll(mask));
        hi = min(hi, lo + step);
    }
    return lo;
}

// Karras node i (wave-cooperative): children and range, as karras_node writes them (parent links are
// not kept: nothing downstream reads them).
__device__ void karras_node_wave(uint32_t n, uint32_t i, const uint32_t* __restrict__ keys, uint32_t* __restrict__ lch,
                                 uint32_t* __restrict__ rch, uint32_t* __restrict__ first,
                                 uint32_t* __restrict__ last) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ki = keys[i];
    auto delta = [&](long long j) -> int {
        if (j < 0 || j >= (long long)n) return -1;
        return kdelta_aug(ki, keys[(uint32_t)j], i, (uint32_t)j);
    };
    const int d = (delta((long long)i + 1) - delta((long long)i - 1)) >= 0 ? 1 : -1;
    const int dmin = delta((long long)i - d);
    // the other end: largest l with delta(i, i + l d) > dmin (l >= 1); exponential bracket, 64-ary refine
    const unsigned long long em = ballot(lane < 31 && delta((long long)i + (long long)d * (1ll << lane)) > dmin);
    const uint32_t a = 63 - __clzll(em);
    const uint32_t l = wave_last_true(1u << a, a >= 31 ? 0xFFFFFFFFu : (2u << a), [&](uint32_t m) {
        return delta((long long)i + (long long)d * m) > dmin;
    });
    const uint32_t j = (uint32_t)((long long)i + (long long)d * l);
    const int dnode = delta(j);
    const uint32_t sp = wave_last_true(0u, l, [&](uint32_t m) { return delta((long long)i + (long long)d * m) > dnode; });
    const uint32_t gamma = (uint32_t)((long long)i + (long long)d * sp + (d < 0 ? -1 : 0));
    if (lane != 0) return;
    const uint32_t lo = min(i, j), hi = max(i, j);
    *(lch + i) = lo == gamma ? (gamma | LEAF_BIT) : gamma;
    *(rch + i) = hi == gamma + 1 ? ((gamma + 1) | LEAF_BIT) : gamma + 1;
    *(first + i) = lo;
    *(last + i) = hi;
}

// Spanning nodes (Karras indices whose range crosses a chunk edge), one lane per index: the test is
// O(1) (delta(i, x) does not grow with the distance of x from i, so the range reaches past the chunk
// edge iff the key beyond it still shares more than dmin bits). About ten per chunk edge, clustered
// around it: a workgroup of SB indices lists its spanning indices in LDS and deals them to its waves,
// which run the searches 64-ary. Each wave also stores its 64-bit ballot into span_bits (its own
// words: no atomics) for k_pack4_span; block 0 folds the scene bounds for the later kernels.
template <int SB>
__device__ __forceinline__ void span_body(uint32_t blk, uint32_t n, const uint32_t* __restrict__ keys,
                                          uint32_t* __restrict__ lch, uint32_t* __restrict__ rch,
                                          uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                          uint32_t* __restrict__ meta, uint32_t* __restrict__ span_bits) {
    static_assert(SB % 64 == 0 && SB <= 1024, "span block: whole waves");
    __shared__ uint32_t s_list[SB];
    __shared__ uint32_t s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    if (blk == 0 && threadIdx.x < BOUNDS_SLOTS) *(meta + threadIdx.x) = fold_slot(meta, threadIdx.x);
    const uint32_t i = blk * SB + threadIdx.x;
    const uint32_t wb = i & ~63u;  // a wave's 64 indices lie in one chunk
    const uint32_t c0 = wb & ~(REFIT_CHUNK - 1), c1 = c0 + REFIT_CHUNK - 1;
    bool sp = false;
    if (i + 1 < n) {
        const uint32_t ki = keys[i], kr = keys[i + 1];
        const int dr = kdelta_aug(ki, kr, i, i + 1);
        const int dl = i > 0 ? kdelta_aug(ki, keys[i - 1], i, i - 1) : -1;
        if (dr - dl >= 0) sp = c1 + 1 < n && kdelta_aug(ki, keys[c1 + 1], i, c1 + 1) > dl;
        else sp = c0 > 0 && kdelta_aug(ki, keys[c0 - 1], i, c0 - 1) > dr;
    }
    const unsigned long long m = ballot(sp);
    const uint32_t lane = threadIdx.x & 63;
    if (lane < 2) *(span_bits + (wb >> 5) + lane) = (uint32_t)(m >> (32 * lane));
    __syncthreads();  // s_cnt zeroed
    if (sp) s_list[atomicAdd(&s_cnt, 1u)] = i;
    __syncthreads();
    const uint32_t cnt = s_cnt;
    for (uint32_t x = threadIdx.x >> 6; x < cnt; x += SB / 64)
        karras_node_wave(n, s_list[x], keys, lch, rch, first, last);
}

__host__ __device__ __forceinline__ uint32_t floor_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }

// Sparse table of whole-chunk unions: level j, entry i = union of chunks [i, i + 2^j).
// Level 0 is the last prefix of each chunk. One workgroup; levels separated by barriers.
__global__ __launch_bounds__(1024) void k_chunk_table(uint32_t n, const int32_t* __restrict__ pre,
                                                      int32_t* __restrict__ table, uint32_t* __restrict__ bounds) {
    clear_replicas(bounds, threadIdx.x, 1024);  // the chunk kernel was their last reader
    const uint32_t nc = (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2;
    for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) {
        const uint32_t end = min(n, (i + 1) << REFIT_CHUNK_LOG2) - 1;
#pragma unroll
        for (int a = 0; a < 6; ++a) table[6 * (size_t)i + a] = pre[6 * (size_t)end + a];
    }
    for (uint32_t j = 1; (1u << j) <= nc; ++j) {
        __syncthreads();  // level j-1 complete (same workgroup: workgroup-scope visibility)
        const int32_t* src = table + 6 * (size_t)(j - 1) * nc;
        int32_t* dst = table + 6 * (size_t)j * nc;
        const uint32_t half = 1u << (j - 1);
        for (uint32_t i = threadIdx.x; i + (1u << j) <= nc; i += blockDim.x) {
            int32_t r[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) r[a] = src[6 * (size_t)i + a];
            box_union(r, src + 6 * (size_t)(i + half));
#pragma unroll
            for (int a = 0; a < 6; ++a) dst[6 * (size_t)i + a] = r[a];
        }
    }
}

// The same table with the levels built in LDS (ping-pong) and only written to global memory: one
// workgroup still, but each level costs an LDS round trip instead of a global one. For up to
// CT_LDS_CHUNKS chunks (1.5M triangles with 512-leaf chunks).
constexpr uint32_t CT_LDS_CHUNKS = 3072;
// Every workgroup of the grid builds the whole table in LDS (a few thousand unions per level) but
// stores only its contiguous slice of each level: one workgroup storing all of it was bound by one
// CU's store rate (0.6 MB for 2,184 chunks).
__global__ __launch_bounds__(1024) void k_chunk_table_lds(uint32_t n, const int32_t* __restrict__ pre,
                                                          int32_t* __restrict__ table, uint32_t* __restrict__ bounds) {
    if (blockIdx.x == 0) clear_replicas(bounds, threadIdx.x, 1024);  // the chunk kernel was their last reader
    BDIAG(7);
    __shared__ int32_t lv[2][CT_LDS_CHUNKS * 6];
    const uint32_t nc = (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2;
    const uint32_t per = (nc + gridDim.x - 1) / gridDim.x;
    const uint32_t s0 = blockIdx.x * per, s1 = min(nc, s0 + per);  // this workgroup's slice
    for (uint32_t i = threadIdx.x; i < nc; i += blockDim.x) {
        const uint32_t end = min(n, (i + 1) << REFIT_CHUNK_LOG2) - 1;
        const bool mine = i >= s0 && i < s1;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int32_t v = pre[6 * (size_t)end + a];
            lv[0][6 * i + a] = v;
            if (mine) table[6 * (size_t)i + a] = v;
        }
    }
    // two levels per barrier: level j from pairs of level j-1 (global only), level j+1 from quads of
    // level j-1 (global and the other LDS buffer, the next pass's source)
    int cur = 0;
    for (uint32_t j = 1; (1u << j) <= nc; j += 2) {
        __syncthreads();
        const int32_t* src = lv[cur];
        int32_t* dst = lv[cur ^ 1];
        int32_t* g1 = table + 6 * (size_t)j * nc;
        int32_t* g2 = table + 6 * (size_t)(j + 1) * nc;
        const uint32_t h = 1u << (j - 1);
        const bool two = (1u << (j + 1)) <= nc;
        for (uint32_t i = threadIdx.x; i + 2 * h <= nc; i += blockDim.x) {
            const bool mine = i >= s0 && i < s1;
            int32_t r[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) r[a] = src[6 * i + a];
            box_union(r, src + 6 * (i + h));
            if (mine)
#pragma unroll
                for (int a = 0; a < 6; ++a) g1[6 * (size_t)i + a] = r[a];
            if (two && i + 4 * h <= nc) {
                box_union(r, src + 6 * (i + 2 * h));
                box_union(r, src + 6 * (i + 3 * h));
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    dst[6 * i + a] = r[a];
                    if (mine) g2[6 * (size_t)i + a] = r[a];
                }
            }
        }
        cur ^= 1;
    }
}

// Box of an internal node from the refit products (see k_tree_chunk).
__device__ __forceinline__ void node_box(uint32_t c, const uint32_t* __restrict__ first,
                                         const uint32_t* __restrict__ last, const int32_t* __restrict__ ibox,
                                         const int32_t* __restrict__ pre, const int32_t* __restrict__ suf,
                                         const int32_t* __restrict__ table, uint32_t nc, int32_t* r);

// Same, with the node's sorted range [f, l] already loaded.
__device__ __forceinline__ void node_box_fl(uint32_t c, uint32_t f, uint32_t l, const int32_t* __restrict__ ibox,
                                            const int32_t* __restrict__ pre, const int32_t* __restrict__ suf,
                                            const int32_t* __restrict__ table, uint32_t nc, int32_t* r) {
    const uint32_t cf = f >> REFIT_CHUNK_LOG2, cl = l >> REFIT_CHUNK_LOG2;
    if (cf == cl) {
#pragma unroll
        for (int a = 0; a < 6; ++a) r[a] = ibox[6 * (size_t)c + a];
        return;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) r[a] = suf[6 * (size_t)f + a];
    box_union(r, pre + 6 * (size_t)l);
    if (cl - cf >= 2) {
        const uint32_t a0 = cf + 1, b0 = cl - 1, j = floor_log2(b0 - a0 + 1);
        const int32_t* lvl = table + 6 * (size_t)j * nc;
        box_union(r, lvl + 6 * (size_t)a0);
        box_union(r, lvl + 6 * (size_t)(b0 + 1 - (1u << j)));
    }
}

__device__ __forceinline__ void node_box(uint32_t c, const uint32_t* __restrict__ first,
                                         const uint32_t* __restrict__ last, const int32_t* __restrict__ ibox,
                                         const int32_t* __restrict__ pre, const int32_t* __restrict__ suf,
                                         const int32_t* __restrict__ table, uint32_t nc, int32_t* r) {
    node_box_fl(c, first[c], last[c], ibox, pre, suf, table, nc, r);
}

__device__ __forceinline__ void pad_box(float* lo, float* hi, float pad) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = lo[c] - (fabsf(lo[c]) * PAD_SCALE + pad);
        hi[c] = hi[c] + (fabsf(hi[c]) * PAD_SCALE + pad);
    }
}

__device__ __forceinline__ float scene_pad(const uint32_t* __restrict__ bounds) {
    const float ex = bounds_hi(bounds[3]) - bounds_lo(bounds[0]);
    const float ey = bounds_hi(bounds[4]) - bounds_lo(bounds[1]);
    const float ez = bounds_hi(bounds[5]) - bounds_lo(bounds[2]);
    return omax(omax(ex, ey), ez) * PAD_SCALE;
}

__device__ __forceinline__ void store_record(uint32_t* rec, const uint32_t (&r)[16]) {
    uint4* q = reinterpret_cast<uint4*>(rec);
    q[0] = make_uint4(r[0], r[1], r[2], r[3]);
    q[1] = make_uint4(r[4], r[5], r[6], r[7]);
    q[2] = make_uint4(r[8], r[9], r[10], r[11]);
    q[3] = make_uint4(r[12], r[13], r[14], r[15]);
}

__device__ __forceinline__ void set_child(uint32_t (&r)[16], int slot, const float* lo, const float* hi, uint32_t ref) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[slot * 6 + c] = f2u(lo[c]);
        r[slot * 6 + 3 + c] = f2u(hi[c]);
    }
    r[12 + slot] = ref;
}

__device__ __forceinline__ void set_empty(uint32_t (&r)[16], int slot) {
#pragma unroll
    for (int c = 0; c < 6; ++c) r[slot * 6 + c] = NAN_BITS;
    r[12 + slot] = EMPTY_REF;
}

__global__ __launch_bounds__(BLOCK) void k_pack(uint32_t n, uint32_t K, const uint32_t* __restrict__ lch,
                                                const uint32_t* __restrict__ rch, const uint32_t* __restrict__ first,
                                                const uint32_t* __restrict__ last, const uint32_t* __restrict__ perm,
                                                const float* __restrict__ aabb, const MeshDesc* __restrict__ meshes,
                                                uint32_t nm, const int32_t* __restrict__ ibox,
                                                const int32_t* __restrict__ pre, const int32_t* __restrict__ suf,
                                                const int32_t* __restrict__ table, const uint32_t* __restrict__ bounds,
                                                uint32_t* __restrict__ records) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n - 1) return;
    const uint32_t nc = (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2;
    uint32_t r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = 0u;
    const uint32_t cnt = last[i] - first[i] + 1;
    if (i != 0 && cnt <= K) {  // collapsed into a leaf of its parent
        store_record(records + 16 * (size_t)i, r);
        return;
    }
    const float pad = scene_pad(bounds);
    if (i == 0 && cnt <= K) {
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = unord(ibox[a]);
            hi[a] = unord(ibox[3 + a]);
        }
        pad_box(lo, hi, pad);
        set_child(r, 0, lo, hi, LEAF_BIT | ((cnt - 1) << 27));
        set_empty(r, 1);
        store_record(records, r);
        return;
    }
    const uint32_t ch[2] = {lch[i], rch[i]};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t c = ch[q], cc = c & ~LEAF_BIT;
        float lo[3], hi[3];
        uint32_t cf, cn;
        if (c & LEAF_BIT) {
            child_box(c, perm, aabb, meshes, nm, ibox, lo, hi);
            cf = cc;
            cn = 1;
        } else {
            int32_t b[6];
            node_box(cc, first, last, ibox, pre, suf, table, nc, b);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = unord(b[a]);
                hi[a] = unord(b[3 + a]);
            }
            cf = first[cc];
            cn = last[cc] - first[cc] + 1;
        }
        pad_box(lo, hi, pad);
        set_child(r, q, lo, hi, cn <= K ? (LEAF_BIT | ((cn - 1) << 27) | cf) : cc);
    }
    store_record(records + 16 * (size_t)i, r);
}

// ---- BVH4 records (128 B): every other level of the binary tree collapsed ---------------------
//   [0..3] lo.x of children 0..3  [4..7] lo.y  [8..11] lo.z  [12..15] hi.x  [16..19] hi.y
//   [20..23] hi.z  [24..27] child refs  [28..31] 0.  Empty slot: NaN box, EMPTY_REF.
// A record is written for the root and for every non-collapsed internal node at even depth; its
// children are its binary children with each non-collapsed internal child replaced by that child's
// two children (oracle/beam_oracle.c orc_bvh_build_ex, width 4). Other slots are left unwritten.
__device__ __forceinline__ void set_child4(uint32_t (&r)[32], int slot, const float* lo, const float* hi,
                                           uint32_t ref) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r[4 * c + slot] = f2u(lo[c]);
        r[12 + 4 * c + slot] = f2u(hi[c]);
    }
    r[24 + slot] = ref;
}

__device__ __forceinline__ void set_empty4(uint32_t (&r)[32], int slot) {
#pragma unroll
    for (int c = 0; c < 6; ++c) r[4 * c + slot] = NAN_BITS;
    r[24 + slot] = EMPTY_REF;
}

__device__ __forceinline__ void store_record4(uint32_t* rec, const uint32_t (&r)[32]) {
    uint4* q = reinterpret_cast<uint4*>(rec);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
}

// LDS of one chunk workgroup (kept under 40 KiB, four workgroups per CU: deltas as bytes, node ranges as
// chunk offsets, the keys over the node boxes, which are written only after the deltas are taken).
struct ChunkLds {
    uint32_t bnd[6];                // scene box slots 0..5 (the records' padding)
    int8_t dl[REFIT_CHUNK + 1];     // delta(j, j+1) for j = c0-1 .. c1, at j - c0 + 1 (-1 .. 64)
    int32_t leaf[REFIT_CHUNK][6];
    int32_t wtot[REFIT_CHUNK / 64][6];
    // arrivals at split gamma (at gamma - c0): the first arrival's (ref, far end of its range | side << 31)
    // exchanged in as one 64-bit word; the second arrival takes it out in the same exchange and leaves
    // SLOT_DONE, so a word still holding an arrival after the growth marks a split reached once
    unsigned long long slot[REFIT_CHUNK];
    // chunk-local internal node c0 + x: children, range, box, parent (written out coalesced at the end,
    // so the growth loop's release atomics wait on LDS traffic only; the parent only decides which)
    uint32_t ncl[REFIT_CHUNK], ncr[REFIT_CHUNK];  // children refs
    uint32_t nlr[REFIT_CHUNK];      // range: (first - c0) | (last - c0) << 16; NO_NODE: not chunk-local
    int32_t nbox[REFIT_CHUNK][6];
    // bits 0-9: chunk offset + 1 of the node's chunk-local parent (0: none); bit 16: leaf x starts a
    // maximal chunk-local subtree, bit 17: ends one
    uint32_t pe[REFIT_CHUNK];
};

// One 512-leaf chunk per workgroup: the chunk-local nodes, their boxes, the sorted triangle records.
// The scene box (for the records' padding) is folded from the gather's replicas here, so the chunk
// workgroups do not wait for the span workgroups' fold (they run beside them: k_span_chunk).
template <class Diag>
__device__ __forceinline__ void chunk_body(const Diag& diag, ChunkLds& L, uint32_t blk, uint32_t n,
                                           const uint32_t* __restrict__ keys,
                                           const uint32_t* __restrict__ perm,
                                           const MeshDesc* __restrict__ meshes, uint32_t nm,
                                           float4* __restrict__ tdst,
                                           uint32_t* __restrict__ lch, uint32_t* __restrict__ rch,
                                           uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                           int32_t* __restrict__ ibox, int32_t* __restrict__ pre,
                                           int32_t* __restrict__ suf, uint32_t* __restrict__ bounds, uint32_t K,
                                           uint32_t* __restrict__ records) {
    uint32_t* const s_bnd = L.bnd;
    if (threadIdx.x < 64) {  // wave 0
        const uint32_t v = fold6_wave(bounds, 0);
        if (threadIdx.x < 6) s_bnd[threadIdx.x] = v;
    }
    if (n <= REFIT_CHUNK && threadIdx.x < BOUNDS_SLOTS)  // one chunk: no span workgroup folds for the later kernels
        bounds[threadIdx.x] = fold_slot(bounds, threadIdx.x);
    int8_t* const s_dl = L.dl;
    int32_t (*const s_leaf)[6] = L.leaf;
    int32_t (*const s_wtot)[6] = L.wtot;
    unsigned long long* const s_slot = L.slot;
    uint32_t* const s_ncl = L.ncl;
    uint32_t* const s_ncr = L.ncr;
    uint32_t* const s_nlr = L.nlr;
    int32_t (*const s_nbox)[6] = L.nbox;
    uint32_t* s_key = reinterpret_cast<uint32_t*>(&s_nbox[0][0]);  // keys c0-1 .. c1+1, until the deltas
    uint32_t* const s_pe = L.pe;
    constexpr uint32_t NO_NODE = 0xFFFFFFFFu, PE_START = 1u << 16, PE_END = 1u << 17, PE_PARENT = 0x3FFu;
    const uint32_t tid = threadIdx.x, c0 = blk * REFIT_CHUNK, c1 = c0 + REFIT_CHUNK - 1;
    const uint32_t k = c0 + tid;
    const int w = tid >> 6, lane = tid & 63;
    s_slot[tid] = SLOT_EMPTY;
    s_pe[tid] = 0;
    s_nlr[tid] = NO_NODE;
    // every load issued before any is waited on: own key, the chunk's outer neighbour keys (clamped;
    // lanes 0 and 1 keep theirs), the permutation, then the box and the record it points at
    const uint32_t kc = min(k, n - 1);
    const long long jn = tid == 0 ? (long long)c0 - 1 : (long long)c1 + 1;
    const uint32_t key_own = keys[kc];
    const uint32_t key_nb = keys[(uint32_t)min(max(jn, 0ll), (long long)n - 1)];
    const uint32_t g = perm[kc];
    int32_t leaf[6];
    float4 t0, t1, t2;
    {
        // the sorted triangle's box and (v0, e1, e2) record straight from the mesh, with k_gather's
        // operations (tri_from_mesh): the same bits as gathered copies, without original-order records'
        // write and their permuted 48 + 24-B re-reads
        vec3f p0, p1, p2;
        tri_from_mesh(meshes, nm, g, p0, p1, p2);
        tri_box_ord(p0, p1, p2, leaf);
        tri_record(p0, p1, p2, g, t0, t1, t2);
    }
    s_key[tid + 1] = key_own;
    if (tid < 2) s_key[tid == 0 ? 0 : REFIT_CHUNK + 1] = (jn >= 0 && jn < (long long)n) ? key_nb : 0u;
    if (k < n) {
        // triangle records into leaf (sorted) order
        tdst[3 * (size_t)k + 0] = t0;
        tdst[3 * (size_t)k + 1] = t1;
        tdst[3 * (size_t)k + 2] = t2;
    } else {
        box_identity(leaf);
    }
    __syncthreads();
    diag.mark(0);
    // adjacent deltas: entry x = delta(c0 - 1 + x, c0 + x), x in [0, 512]
    for (uint32_t x = tid; x <= REFIT_CHUNK; x += REFIT_CHUNK) {
        const long long j = (long long)c0 - 1 + x;
        s_dl[x] = (int8_t)((j < 0 || j + 1 >= (long long)n) ? -1 : kdelta_aug(s_key[x], s_key[x + 1], (uint32_t)j, (uint32_t)j + 1));
    }
    // inclusive prefix and suffix unions over the chunk
    int32_t pf[6], sf[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        pf[a] = leaf[a];
        sf[a] = leaf[a];
        s_leaf[tid][a] = leaf[a];
    }
    // within each row of 16 lanes by DPP row shifts (lanes shifted in from outside the row keep the
    // identity), across the four rows by the rows' totals (readlane) — no LDS-crossbar round trips
    // (a wave scan by shuffles takes six dependent steps of twelve)
    {
        const int row = (int)(lane >> 4);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const int32_t id = a < 3 ? INT_MAX : INT_MIN;
            auto op = [&](int32_t x, int32_t y) { return a < 3 ? min(x, y) : max(x, y); };
            int32_t v = pf[a], u = sf[a];
            v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false));  // row_shr:1
            v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false));  // row_shr:2
            v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false));  // row_shr:4
            v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false));  // row_shr:8
            u = op(u, __builtin_amdgcn_update_dpp(id, u, 0x101, 0xf, 0xf, false));  // row_shl:1
            u = op(u, __builtin_amdgcn_update_dpp(id, u, 0x102, 0xf, 0xf, false));  // row_shl:2
            u = op(u, __builtin_amdgcn_update_dpp(id, u, 0x104, 0xf, 0xf, false));  // row_shl:4
            u = op(u, __builtin_amdgcn_update_dpp(id, u, 0x108, 0xf, 0xf, false));  // row_shl:8
            const int32_t t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31);
            const int32_t t2 = __builtin_amdgcn_readlane(v, 47), t3 = __builtin_amdgcn_readlane(v, 63);
            const int32_t p01 = op(t0, t1), s23 = op(t2, t3);
            const int32_t pre = row == 0 ? id : row == 1 ? t0 : row == 2 ? p01 : op(p01, t2);
            const int32_t suf = row == 3 ? id : row == 2 ? t3 : row == 1 ? s23 : op(t1, s23);
            pf[a] = op(v, pre);
            sf[a] = op(u, suf);
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int a = 0; a < 6; ++a) s_wtot[w][a] = pf[a];
    }
    __syncthreads();
    diag.mark(1);
    for (int q = 0; q < REFIT_CHUNK / 64; ++q) {
        if (q < w) box_union(pf, s_wtot[q]);
        if (q > w) box_union(sf, s_wtot[q]);
    }
    if (k < n) {
        // bottom-up growth from leaf k. Per level: one 64-bit exchange at the split (release: this
        // node's box is in LDS before its sibling can read it; acquire: the sibling's is), then the
        // sibling's box and the one new adjacent delta read together.
        uint32_t l = k, r = k, ref = LEAF_BIT | k, cl = 0, cr = 0;
        int32_t box[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) box[a] = leaf[a];
        bool internal = false;
        int dl_r = s_dl[r - c0 + 1], dl_l = s_dl[l - c0];  // delta(r, r+1), delta(l-1, l)
        for (;;) {
            const bool root = l == 0 && r == n - 1;
            const bool right = !root && dl_r > dl_l;  // parent to the right: left child
            if (internal) {
                const uint32_t idx = root ? 0u : (right ? r : l);
                s_ncl[idx - c0] = cl;
                s_ncr[idx - c0] = cr;
                s_nlr[idx - c0] = (l - c0) | ((r - c0) << 16);
#pragma unroll
                for (int a = 0; a < 6; ++a) s_nbox[idx - c0][a] = box[a];
                if (!(cl & LEAF_BIT)) atomicOr(&s_pe[cl - c0], idx - c0 + 1);
                if (!(cr & LEAF_BIT)) atomicOr(&s_pe[cr - c0], idx - c0 + 1);
                ref = idx;
            }
            if (root || (right ? r >= c1 : l <= c0)) {  // the parent's range leaves the chunk: maximal
                atomicOr(&s_pe[l - c0], PE_START);
                atomicOr(&s_pe[r - c0], PE_END);
                break;
            }
            const uint32_t gi = (right ? r : l - 1) - c0;
            const unsigned long long mine =
                ((unsigned long long)((right ? l : r) | (right ? 0u : 0x80000000u)) << 32) | ref;
            const unsigned long long prev =
                __hip_atomic_exchange(&s_slot[gi], mine, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (prev == SLOT_EMPTY) break;  // first arrival: the sibling continues
            s_slot[gi] = SLOT_DONE;
            const uint32_t sref = (uint32_t)prev, send = (uint32_t)(prev >> 32) & 0x7FFFFFFFu;
            const int32_t* sb = (sref & LEAF_BIT) ? s_leaf[(sref & ~LEAF_BIT) - c0] : s_nbox[sref - c0];
            if (right) {
                cl = ref;
                cr = sref;
                r = send;
                dl_r = s_dl[r - c0 + 1];
            } else {
                cl = sref;
                cr = ref;
                l = send;
                dl_l = s_dl[l - c0];
            }
            box_union(box, sb);
            internal = true;
        }
    }
    __syncthreads();
    diag.mark(2);
    {  // chunk-local nodes out, coalesced (the spanning ones are written by span_body). With BVH4 records
       // written here, k_pack4_span reads only the top two levels of each maximal subtree (children
       // and grandchildren of spanning nodes); BVH2's k_pack reads every node.
        const uint32_t lr = s_nlr[tid];
        if (lr != NO_NODE) {
            const uint32_t pp = s_pe[tid] & PE_PARENT;
            if (!records || pp == 0 || (s_pe[pp - 1] & PE_PARENT) == 0) {
                *(lch + k) = s_ncl[tid];
                *(rch + k) = s_ncr[tid];
                *(first + k) = c0 + (lr & 0xFFFFu);
                *(last + k) = c0 + (lr >> 16);
#pragma unroll
                for (int a = 0; a < 6; ++a) *(ibox + 6 * (size_t)k + a) = s_nbox[tid][a];
            }
        }
    }
    // a split reached by one child only: its parent spans chunks, so that child is maximal too
    const unsigned long long once = s_slot[tid];
    if (once != SLOT_EMPTY && once != SLOT_DONE) {
        const uint32_t sd = (uint32_t)(once >> 63), far = (uint32_t)(once >> 32) & 0x7FFFFFFFu;
        atomicOr(&s_pe[sd == 0 ? far - c0 : tid + 1], PE_START);
        atomicOr(&s_pe[sd == 0 ? tid : far - c0], PE_END);
    }
    __syncthreads();
    diag.mark(3);
    // a spanning node's box is suf[its first leaf] U whole chunks U pre[its last leaf], and those leaves
    // are ends of maximal chunk-local subtrees: only there are the prefix/suffix unions needed
    if (k < n) {
        const uint32_t e = (s_pe[tid] >> 16) & 3u;
        if (e & 1u) {
#pragma unroll
            for (int a = 0; a < 6; ++a) *(suf + 6 * (size_t)k + a) = sf[a];
        }
        if (e & 2u) {
#pragma unroll
            for (int a = 0; a < 6; ++a) *(pre + 6 * (size_t)k + a) = pf[a];
        }
    }
    if (n <= REFIT_CHUNK) clear_replicas(bounds, tid, REFIT_CHUNK);  // one chunk: their last reader was above
    if (!records) return;  // BVH2: k_pack writes every record
    // BVH4 record of every chunk-local node above the leaf size (the spanning ones: k_pack4_span).
    // A traversal reaches only the records of nodes at even depth (the others are expanded into
    // their parents' records), but a node's record does not depend on its depth, so writing all of
    // them needs no depth (which only a top-down pass over the spanning nodes could supply) and
    // leaves every reachable record as the oracle's.
    const uint32_t lr = s_nlr[tid];
    if (lr == NO_NODE) return;
    const uint32_t cnt = (lr >> 16) - (lr & 0xFFFFu) + 1;
    if (cnt <= K && k != 0) return;  // inside a leaf
    const float pad = scene_pad(s_bnd);
    // slots in record order: child 0 (or its two children if expanded), then child 1 (or its two)
    uint32_t sl[4] = {EMPTY_REF, EMPTY_REF, EMPTY_REF, EMPTY_REF};
    if (cnt <= K) {  // the whole scene is one leaf: the root's own box
        sl[0] = k;
    } else {
        bool ex[2];
        uint32_t cc[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint32_t c = q ? s_ncr[tid] : s_ncl[tid];
            const uint32_t clr = (c & LEAF_BIT) ? 0u : s_nlr[c - c0];
            ex[q] = !(c & LEAF_BIT) && (clr >> 16) - (clr & 0xFFFFu) + 1 > K;
            cc[q][0] = ex[q] ? s_ncl[c - c0] : c;
            cc[q][1] = ex[q] ? s_ncr[c - c0] : EMPTY_REF;
        }
        sl[0] = cc[0][0];
        sl[1] = ex[0] ? cc[0][1] : cc[1][0];
        sl[2] = ex[0] ? cc[1][0] : cc[1][1];
        sl[3] = ex[0] ? cc[1][1] : EMPTY_REF;
    }
    uint32_t rr[32];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t c = sl[q];
        if (c == EMPTY_REF) {
            set_empty4(rr, q);
            continue;
        }
        const int32_t* ob = (c & LEAF_BIT) ? s_leaf[(c & ~LEAF_BIT) - c0] : s_nbox[c - c0];
        float b[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = unord(ob[a]);
        uint32_t ref = c;
        if (!(c & LEAF_BIT)) {
            const uint32_t clr = s_nlr[c - c0];
            const uint32_t gn = (clr >> 16) - (clr & 0xFFFFu) + 1;
            if (gn <= K) ref = LEAF_BIT | ((gn - 1) << 27) | (c0 + (clr & 0xFFFFu));
        }
        pad_box(b, b + 3, pad);
        set_child4(rr, q, b, b + 3, ref);
    }
#pragma unroll
    for (int q = 28; q < 32; ++q) rr[q] = 0u;
    store_record4(records + 32 * (size_t)k, rr);
}

__global__ __launch_bounds__(REFIT_CHUNK) void k_tree_chunk(uint32_t n, const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ perm,
                                                            const MeshDesc* __restrict__ meshes, uint32_t nm,
                                                            float4* __restrict__ tdst,
                                                            uint32_t* __restrict__ lch, uint32_t* __restrict__ rch,
                                                            uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                            int32_t* __restrict__ ibox,
                                                            int32_t* __restrict__ pre, int32_t* __restrict__ suf,
                                                            uint32_t* __restrict__ bounds, uint32_t K,
                                                            uint32_t* __restrict__ records) {
    BDIAG(6);
    __shared__ ChunkLds L;
    chunk_body(BDIAG_OBJ, L, blockIdx.x, n, keys, perm, meshes, nm, tdst, lch, rch, first, last, ibox, pre,
               suf, bounds, K, records);
}

// span_body and chunk_body in one launch (more than one chunk): workgroups [0, nchunk) grow the chunks,
// the rest find and search the spanning nodes (512 indices each). The two only read the sorted keys and
// write disjoint nodes, so they overlap instead of paying a launch boundary and the searches' span.
__global__ __launch_bounds__(REFIT_CHUNK) void k_span_chunk(uint32_t nchunk, uint32_t n, const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ perm,
                                                            const MeshDesc* __restrict__ meshes, uint32_t nm,
                                                            float4* __restrict__ tdst,
                                                            uint32_t* __restrict__ lch, uint32_t* __restrict__ rch,
                                                            uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                            int32_t* __restrict__ ibox,
                                                            int32_t* __restrict__ pre, int32_t* __restrict__ suf,
                                                            uint32_t* __restrict__ bounds, uint32_t K,
                                                            uint32_t* __restrict__ records, uint32_t* __restrict__ span_bits) {
    __shared__ ChunkLds L;
    if (blockIdx.x < nchunk) {
        BDIAG(6);
        chunk_body(BDIAG_OBJ, L, blockIdx.x, n, keys, perm, meshes, nm, tdst, lch, rch, first, last, ibox,
                   pre, suf, bounds, K, records);
    } else {
        BDIAG(5);
        span_body<REFIT_CHUNK>(blockIdx.x - nchunk, n, keys, lch, rch, first, last, bounds, span_bits);
    }
}

// BVH4 records of the spanning nodes (span_body's bitmap: about ten per chunk edge), four lanes per
// record, lane c building slot c. A record is latency-bound — children, their ranges and children,
// the slot nodes' ranges or triangle ids, then up to four boxes per slot (a spanning slot: suffix,
// prefix, two table entries) — so the lanes of a record run those rounds side by side instead of one
// lane running all four slots (about 3,000 instructions: 15 us per record at one wave per CU).
// One 256-thread workgroup per 1024 indices (32 bitmap words): records dealt 64 per round.
constexpr uint32_t PACK4_IDX = 1024;
// The records of window `win` (PACK4_IDX indices) by BLOCK threads, tid = 0 .. BLOCK - 1 (whole waves).
__device__ __forceinline__ void pack4_body(uint32_t win, uint32_t tid, uint32_t n, uint32_t K,
                                           const uint32_t* __restrict__ span_bits, const uint32_t* __restrict__ lch,
                                           const uint32_t* __restrict__ rch, const uint32_t* __restrict__ first,
                                           const uint32_t* __restrict__ last, const uint32_t* __restrict__ perm,
                                           const float* __restrict__ aabb, const MeshDesc* __restrict__ meshes,
                                           uint32_t nm, const int32_t* __restrict__ ibox,
                                           const int32_t* __restrict__ pre, const int32_t* __restrict__ suf,
                                           const int32_t* __restrict__ table, const uint32_t* __restrict__ bounds,
                                           uint32_t* __restrict__ records) {
    const uint32_t lane = tid & 63, c = tid & 3;
    // every wave: the workgroup's 32 bitmap words in lanes 0..31 and their inclusive popcount prefix
    const uint32_t q = win * (PACK4_IDX / 32) + lane;
    const uint32_t nw = (n - 1 + 31) >> 5;
    const uint32_t word = (lane < PACK4_IDX / 32 && q < nw) ? *(span_bits + q) : 0u;
    const uint32_t pc = __popc(word);
    const uint32_t incl = wave_incl_add(pc);  // (lanes 32..63 hold no words: their sums are the total)
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 31);
    const uint32_t nc = (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2;
    const float pad = scene_pad(bounds);
    for (uint32_t r0 = 0; r0 < total; r0 += BLOCK / 4) {
        const uint32_t want = r0 + (tid >> 2);  // this lane's record: the want-th set bit
        uint32_t lo = 0;  // word holding it: the first lane whose inclusive count exceeds want
#pragma unroll
        for (uint32_t step = 16; step >= 1; step >>= 1) {
            const uint32_t v = __shfl(incl, lo + step - 1);
            if (v <= want) lo += step;
        }
        const uint32_t wq = __shfl(word, lo), before = __shfl(incl, lo) - __shfl(pc, lo);
        if (want >= total) continue;
        uint32_t bits = wq;
        for (uint32_t skip = want - before; skip; --skip) bits &= bits - 1;
        const uint32_t i = win * PACK4_IDX + 32 * lo + (uint32_t)__ffs(bits) - 1;
        // round 1-2: the node's children, then each internal child's range and children (a spanning
        // node holds more than 512 > K triangles: never a leaf, always a record)
        const uint32_t ch0 = *(lch + i), ch1 = *(rch + i);
        const uint32_t c0 = (ch0 & LEAF_BIT) ? 0u : ch0, c1 = (ch1 & LEAF_BIT) ? 0u : ch1;
        const uint32_t f0 = *(first + c0), l0 = *(last + c0), g0l = *(lch + c0), g0r = *(rch + c0);
        const uint32_t f1 = *(first + c1), l1 = *(last + c1), g1l = *(lch + c1), g1r = *(rch + c1);
        const bool ex0 = !(ch0 & LEAF_BIT) && l0 - f0 + 1 > K, ex1 = !(ch1 & LEAF_BIT) && l1 - f1 + 1 > K;
        // slots in record order: child 0 (or its two children), then child 1 (or its two)
        const uint32_t n0 = ex0 ? 2u : 1u, used = n0 + (ex1 ? 2u : 1u);
        uint32_t cand = EMPTY_REF;
        if (c < n0) cand = ex0 ? (c == 0 ? g0l : g0r) : ch0;
        else if (c < used) cand = ex1 ? (c == n0 ? g1l : g1r) : ch1;
        // round 3: a triangle slot's sorted position -> id; a node slot's range
        const bool use = cand != EMPTY_REF, leaf = use && (cand & LEAF_BIT);
        const uint32_t gc = cand & ~LEAF_BIT;
        const uint32_t pm = perm[leaf ? gc : 0u];
        const uint32_t nd = (use && !leaf) ? gc : 0u;
        const uint32_t f = *(first + nd), l = *(last + nd);
        // round 4: the slot's boxes, all issued before any is used
        const int32_t* src[4] = {nullptr, nullptr, nullptr, nullptr};
        int parts = 0;
        int32_t bx[4][6];
        const bool mesh_leaf = leaf && !aabb;  // the slot's box from its mesh (mesh-direct builds: no aabb[])
        if (mesh_leaf) {  // as float bits, straight into bx[0] (no pointer to a local array: no scratch)
            vec3f p0, p1, p2;
            tri_from_mesh(meshes, nm, pm, p0, p1, p2);
            tri_box_ord(p0, p1, p2, bx[0]);
#pragma unroll
            for (int a = 0; a < 6; ++a) bx[0][a] = f2i(unord(bx[0][a]));
            parts = 1;
        } else if (leaf) {
            src[0] = reinterpret_cast<const int32_t*>(aabb + 6 * (size_t)pm);
            parts = 1;
        } else if (use) {
            const uint32_t k0 = f >> REFIT_CHUNK_LOG2, k1 = l >> REFIT_CHUNK_LOG2;
            if (k0 == k1) {
                src[0] = ibox + 6 * (size_t)gc;
                parts = 1;
            } else {
                src[0] = suf + 6 * (size_t)f;
                src[1] = pre + 6 * (size_t)l;
                parts = 2;
                if (k1 - k0 >= 2) {
                    const uint32_t a0 = k0 + 1, b0 = k1 - 1, j = floor_log2(b0 - a0 + 1);
                    const int32_t* lvl = table + 6 * (size_t)j * nc;
                    src[2] = lvl + 6 * (size_t)a0;
                    src[3] = lvl + 6 * (size_t)(b0 + 1 - (1u << j));
                    parts = 4;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (m < parts && !(m == 0 && mesh_leaf)) {
                const int2 x0 = *reinterpret_cast<const int2*>(src[m]), x1 = *reinterpret_cast<const int2*>(src[m] + 2), x2 = *reinterpret_cast<const int2*>(src[m] + 4);
                bx[m][0] = x0.x;
                bx[m][1] = x0.y;
                bx[m][2] = x1.x;
                bx[m][3] = x1.y;
                bx[m][4] = x2.x;
                bx[m][5] = x2.y;
            }
        }
        uint32_t out[7];
        if (use) {
            int32_t ob[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) ob[a] = bx[0][a];
#pragma unroll
            for (int m = 1; m < 4; ++m)
                if (m < parts) box_union(ob, bx[m]);
            float b[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) b[a] = leaf ? i2f(ob[a]) : unord(ob[a]);
            const uint32_t gn = l - f + 1;
            pad_box(b, b + 3, pad);
#pragma unroll
            for (int a = 0; a < 6; ++a) out[a] = f2u(b[a]);
            out[6] = leaf ? (LEAF_BIT | gc) : gn <= K ? (LEAF_BIT | ((gn - 1) << 27) | f) : gc;
        } else {
#pragma unroll
            for (int a = 0; a < 6; ++a) out[a] = NAN_BITS;
            out[6] = EMPTY_REF;
        }
        // lane c owns dword c of each 16-B plane: lo.x lo.y lo.z hi.x hi.y hi.z refs 0
        uint32_t* rec = records + 32 * (size_t)i + c;
#pragma unroll
        for (int a = 0; a < 7; ++a) rec[4 * a] = out[a];
        rec[28] = 0u;
    }
}

__global__ __launch_bounds__(BLOCK) void k_pack4_span(uint32_t n, uint32_t K, const uint32_t* __restrict__ span_bits,
                                                      const uint32_t* __restrict__ lch, const uint32_t* __restrict__ rch,
                                                      const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ last,
                                                      const uint32_t* __restrict__ perm, const float* __restrict__ aabb,
                                                       const MeshDesc* __restrict__ meshes, uint32_t nm,
                                                      const int32_t* __restrict__ ibox, const int32_t* __restrict__ pre,
                                                      const int32_t* __restrict__ suf, const int32_t* __restrict__ table,
                                                      const uint32_t* __restrict__ bounds,
                                                      uint32_t* __restrict__ records) {
    BDIAG(8);
    pack4_body(blockIdx.x, threadIdx.x, n, K, span_bits, lch, rch, first, last, perm, aabb, meshes, nm, ibox, pre, suf,
               table, bounds, records);
}

// Up to PT_MAX_CHUNKS chunks (BVH4): no chunk-table launch — each k_pack4_table workgroup builds
// the sparse table of chunk unions (k_chunk_table's levels, same unions in the same order) in its own
// LDS, ~1 us for the bunny's 136 chunks, and answers its spanning records' range queries from there;
// workgroup 0 clears the gather replicas (the chunk kernel was their last reader).
constexpr uint32_t PT_MAX_CHUNKS = 256, PT_LEVELS = 9;  // levels j with 2^j <= 256
__global__ __launch_bounds__(BLOCK) void k_pack4_table(uint32_t n, uint32_t K, const uint32_t* __restrict__ span_bits,
                                                       const uint32_t* __restrict__ lch, const uint32_t* __restrict__ rch,
                                                       const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ last,
                                                       const uint32_t* __restrict__ perm, const float* __restrict__ aabb,
                                                       const MeshDesc* __restrict__ meshes, uint32_t nm,
                                                       const int32_t* __restrict__ ibox, const int32_t* __restrict__ pre,
                                                       const int32_t* __restrict__ suf, uint32_t* __restrict__ bounds,
                                                       uint32_t* __restrict__ records) {
    BDIAG(8);
    __shared__ int32_t lt[PT_LEVELS * PT_MAX_CHUNKS * 6];
    if (blockIdx.x == 0) clear_replicas(bounds, threadIdx.x, BLOCK);
    const uint32_t nc = (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2;
    for (uint32_t i = threadIdx.x; i < nc; i += BLOCK) {
        const uint32_t end = min(n, (i + 1) << REFIT_CHUNK_LOG2) - 1;
#pragma unroll
        for (int a = 0; a < 6; ++a) lt[6 * i + a] = pre[6 * (size_t)end + a];
    }
    for (uint32_t j = 1; (1u << j) <= nc; ++j) {
        __syncthreads();
        const int32_t* src = lt + 6 * (j - 1) * nc;
        int32_t* dst = lt + 6 * j * nc;
        const uint32_t h = 1u << (j - 1);
        for (uint32_t i = threadIdx.x; i + (1u << j) <= nc; i += BLOCK) {
            int32_t r[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) r[a] = src[6 * i + a];
            box_union(r, src + 6 * (i + h));
#pragma unroll
            for (int a = 0; a < 6; ++a) dst[6 * i + a] = r[a];
        }
    }
    __syncthreads();
    pack4_body(blockIdx.x, threadIdx.x, n, K, span_bits, lch, rch, first, last, perm, aabb, meshes, nm, ibox, pre, suf,
               lt, bounds, records);
}

// n <= 1: a single record whose child 0 is the lone triangle (or empty).
__global__ void k_pack_small(uint32_t n, uint32_t width, const float* __restrict__ aabb,
                             uint32_t* __restrict__ bounds, uint32_t* __restrict__ records) {
    for (int t = 0; t < BOUNDS_SLOTS; ++t) bounds[t] = fold_slot(bounds, t);
    clear_replicas(bounds, 0, 1);
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    if (n == 1) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = aabb[a];
            hi[a] = aabb[3 + a];
        }
        pad_box(lo, hi, scene_pad(bounds));
    }
    if (width == 4) {
        uint32_t r[32];
        for (int q = 0; q < 32; ++q) r[q] = 0u;
        if (n == 1) set_child4(r, 0, lo, hi, LEAF_BIT);
        else set_empty4(r, 0);
        for (int q = 1; q < 4; ++q) set_empty4(r, q);
        store_record4(records, r);
        return;
    }
    uint32_t r[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) r[q] = 0u;
    if (n == 1) set_child(r, 0, lo, hi, LEAF_BIT);
    else set_empty(r, 0);
    set_empty(r, 1);
    store_record(records, r);
}

__global__ __launch_bounds__(BLOCK) void k_sort_tris(uint32_t n, const uint32_t* __restrict__ perm,
                                                     const float4* __restrict__ src, float4* __restrict__ dst) {
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t g = perm[k];
    dst[3 * k + 0] = src[3 * g + 0];
    dst[3 * k + 1] = src[3 * g + 1];
    dst[3 * k + 2] = src[3 * g + 2];
}

// BVH8 records (256 B: lo.x[8] lo.y[8] lo.z[8] hi.x[8] hi.y[8] hi.z[8] refs[8] 0[8]) collapsed from
// the BVH2 records: record i lists the frontier three binary levels below node i — its children,
// each non-collapsed internal one replaced by its children, twice — in child order, with the padded
// boxes and refs of the BVH2 records (oracle/beam_oracle.c, width 8). Written for every node (a
// traversal reaches those at depths divisible by three; the others are never read); a BVH2 record
// of zeros (a node collapsed into its parent's leaf) gives zeros.
__global__ __launch_bounds__(BLOCK) void k_pack8(uint32_t nrec, const uint32_t* __restrict__ rec2,
                                                 uint32_t* __restrict__ rec8) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nrec) return;
    const uint32_t* r = rec2 + 16 * (size_t)i;
    uint32_t* o = rec8 + 64 * (size_t)i;
    uint32_t out[64];
#pragma unroll
    for (int q = 0; q < 64; ++q) out[q] = 0u;
    const bool zero = r[12] == 0u && r[13] == 0u && r[0] == 0u && r[6] == 0u;
    if (!zero) {
        // frontier entries: (BVH2 record holding the entry, its slot there)
        uint32_t frec[8], fslot[8], nf = 0;
        for (uint32_t q = 0; q < 2; ++q)
            if (r[12 + q] != EMPTY_REF) {
                frec[nf] = i;
                fslot[nf++] = q;
            }
        for (int e = 0; e < 2; ++e) {
            uint32_t nrec_[8], nslot_[8], nn = 0;
            for (uint32_t k = 0; k < nf; ++k) {
                const uint32_t ref = rec2[16 * (size_t)frec[k] + 12 + fslot[k]];
                if (!(ref & LEAF_BIT)) {  // a non-collapsed internal node: its two children
                    nrec_[nn] = ref;
                    nslot_[nn++] = 0;
                    nrec_[nn] = ref;
                    nslot_[nn++] = 1;
                } else {
                    nrec_[nn] = frec[k];
                    nslot_[nn++] = fslot[k];
                }
            }
            for (uint32_t k = 0; k < nn; ++k) {
                frec[k] = nrec_[k];
                fslot[k] = nslot_[k];
            }
            nf = nn;
        }
        for (uint32_t k = 0; k < 8; ++k) {
            if (k < nf) {
                const uint32_t* c = rec2 + 16 * (size_t)frec[k];
                const uint32_t q = fslot[k];
                for (int a = 0; a < 3; ++a) {
                    out[8 * a + k] = c[6 * q + a];
                    out[24 + 8 * a + k] = c[6 * q + 3 + a];
                }
                out[48 + k] = c[12 + q];
            } else {
                for (int a = 0; a < 6; ++a) out[8 * a + k] = NAN_BITS;
                out[48 + k] = EMPTY_REF;
            }
        }
    }
    uint4* o4 = reinterpret_cast<uint4*>(o);
#pragma unroll
    for (int q = 0; q < 16; ++q) o4[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}

}  // namespace


// The bucket plan (bucket_plan) follows the look-back words, outside the block k_gather zero-fills (it is
// written whole before k_bucket_sort reads it).
static size_t plan_offset(uint32_t n) { return META_LOOKBACK + (size_t)RADIX_PASSES * onesweep_tiles(n) * RADIX; }
size_t build_meta_words(uint32_t n) { return plan_offset(n) + PLAN_WORDS; }

// What one k_gather launch writes: the scene bounds (needs META_GATHER_CLEAR zeroed words), original-order
// records (tri_orig), corner normals, AABBs, AABB centres
enum GatherOut : unsigned { G_BOUNDS = 1, G_TRI = 2, G_NRM = 4, G_AABB = 8, G_CEN = 16 };
// triangles -> the outputs in `out`; zero-fills meta words [clear_begin, clear_end)
static void launch_gather_kernel(const BuildBuffers& b, hipStream_t s, unsigned out, uint32_t clear_begin = 0,
                                 uint32_t clear_end = 0) {
    k_gather<<<blocks_for(b.n, BLOCK), BLOCK, 0, s>>>(b.meshes, b.num_meshes, b.n, b.tri_orig, b.nrm,
                                                     (out & G_AABB) ? b.aabb : nullptr, (out & G_CEN) ? b.cen : nullptr,
                                                     b.bounds, clear_begin, clear_end, (out & G_BOUNDS) ? 1 : 0,
                                                     (out & G_TRI) ? 1 : 0, (out & G_NRM) ? 1 : 0);
}
uint32_t num_records(uint32_t n) { return n > 1 ? n - 1 : 1; }

size_t sort_meta_words(uint32_t n, int key_bits) {
    const int passes = (key_bits + RADIX_BITS - 1) / RADIX_BITS;
    const uint32_t nb = onesweep_tiles(n);
    return 4 + (size_t)passes * RADIX + (size_t)passes * nb * RADIX;
}
size_t chunk_table_floats(uint32_t n) {
    const uint32_t nc = n ? (n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2 : 1;
    return (size_t)6 * nc * (floor_log2(nc) + 1);
}

#define BM_LAUNCH_CHECK()                          \
    do {                                           \
        hipError_t e_ = hipGetLastError();         \
        if (e_ != hipSuccess) return e_;           \
    } while (0)

// Shared by build and refit: bottom-up boxes over the current topology, node records, sorted
// triangle records. Needs gather (aabb, bounds, tri_orig) and the topology (vals, tree arrays).
// the refit products (ibox, pre, suf, table) hold ordered-int box images (see box_union)
inline int32_t* ob(float* p) { return reinterpret_cast<int32_t*>(p); }

// The chunk kernel and the record writers read each sorted triangle from its mesh (tri_from_mesh), so a
// build writes the gather's per-triangle arrays only where something else reads them.
// Original-order records (tri_orig): a multi-device root reshades from them (launch_reshade) and the
// one-triangle path sorts them (k_sort_tris).
static bool need_orig(const BuildBuffers& b) { return b.orig_records || b.n == 1; }
// Per-triangle AABBs (aabb[]): only the one-triangle path (k_pack_small) reads them; the Morton keys come
// from the gather's AABB centres (cen[], 12 B instead of 24).
static bool need_aabb(const BuildBuffers& b) { return b.n == 1; }

// BVH8: the BVH2 records (into records2), then k_pack8 collapses them into records.
static hipError_t launch_pack8(const BuildBuffers& b, hipStream_t s) {
    const uint32_t nrec = b.n > 1 ? b.n - 1 : 1;
    k_pack8<<<blocks_for(nrec, BLOCK), BLOCK, 0, s>>>(nrec, b.records2, b.records);
    BM_LAUNCH_CHECK();
    return hipSuccess;
}

// The empty scene (build and refit alike, after their zero fill): the single empty record.
static hipError_t launch_empty(const BuildBuffers& b, hipStream_t s) {
    k_pack_small<<<1, 1, 0, s>>>(0, b.width == 8 ? 2u : b.width, b.aabb, b.bounds,
                                 b.width == 8 ? b.records2 : b.records);
    BM_LAUNCH_CHECK();
    return b.width == 8 ? launch_pack8(b, s) : hipSuccess;
}

constexpr uint32_t CT_SPLIT_CHUNKS = 512;  // from this many chunks the LDS table's stores are split over 8 workgroups
static hipError_t launch_finish(const BuildBuffers& b, hipStream_t s) {
    const uint32_t n = b.n;
    const bool w8 = b.width == 8;
    uint32_t* rec2 = w8 ? b.records2 : b.records;  // where the BVH2 (or small-scene) records go
    if (n == 1) {
        k_pack_small<<<1, 1, 0, s>>>(1, w8 ? 2u : b.width, b.aabb, b.bounds, rec2);
        BM_LAUNCH_CHECK();
        k_sort_tris<<<1, BLOCK, 0, s>>>(n, b.vals, b.tri_orig, b.tris);
        BM_LAUNCH_CHECK();
        return w8 ? launch_pack8(b, s) : hipSuccess;
    }
    // the sort's scratch is free again: vals2 holds the spanning bitmap
    uint32_t* span_bits = b.vals2;
    const bool w4 = b.width == 4;
    const uint32_t nchunk = blocks_for(n, REFIT_CHUNK);
    // the record writers' per-triangle box array: no build past one triangle keeps one (need_aabb), so
    // they take every leaf's box from its mesh
    const float* const no_aabb = nullptr;
    if (n > REFIT_CHUNK) {
        // the spanning nodes' searches as further workgroups of the chunk launch: measured faster than a
        // launch of their own at every size (bunny 0.089 -> 0.080 ms, armadillo proxy 0.131 -> 0.122, 1.1M
        // merged 0.270 -> 0.264)
        k_span_chunk<<<nchunk + blocks_for(n - 1, REFIT_CHUNK), REFIT_CHUNK, 0, s>>>(
            nchunk, n, b.keys, b.vals, b.meshes, b.num_meshes, b.tris, b.lch, b.rch, b.first, b.last, ob(b.ibox),
            ob(b.pre), ob(b.suf), b.bounds, b.leaf_size, w4 ? b.records : nullptr, span_bits);
    } else {  // one chunk: no spanning nodes
        k_tree_chunk<<<nchunk, REFIT_CHUNK, 0, s>>>(n, b.keys, b.vals, b.meshes, b.num_meshes, b.tris, b.lch, b.rch,
                                                    b.first, b.last, ob(b.ibox), ob(b.pre), ob(b.suf), b.bounds,
                                                    b.leaf_size, w4 ? b.records : nullptr);
    }
    BM_LAUNCH_CHECK();
    if (n > REFIT_CHUNK && w4 && nchunk <= PT_MAX_CHUNKS) {
        k_pack4_table<<<blocks_for(n - 1, PACK4_IDX), BLOCK, 0, s>>>(n, b.leaf_size, span_bits, b.lch, b.rch, b.first,
                                                                    b.last, b.vals, no_aabb, b.meshes,
                                                                    b.num_meshes, ob(b.ibox), ob(b.pre),
                                                                    ob(b.suf), b.bounds, b.records);
        BM_LAUNCH_CHECK();
    } else if (n > REFIT_CHUNK) {
        if (((n + REFIT_CHUNK - 1) >> REFIT_CHUNK_LOG2) <= CT_LDS_CHUNKS)
            k_chunk_table_lds<<<nchunk >= CT_SPLIT_CHUNKS ? 8 : 1, 1024, 0, s>>>(n, ob(b.pre), ob(b.table), b.bounds);
        else
            k_chunk_table<<<1, 1024, 0, s>>>(n, ob(b.pre), ob(b.table), b.bounds);
        BM_LAUNCH_CHECK();
        if (w4) {
            k_pack4_span<<<blocks_for(n - 1, PACK4_IDX), BLOCK, 0, s>>>(n, b.leaf_size, span_bits, b.lch, b.rch,
                                                                   b.first, b.last, b.vals, no_aabb, b.meshes,
                                                                   b.num_meshes, ob(b.ibox),
                                                                   ob(b.pre), ob(b.suf), ob(b.table), b.bounds,
                                                                   b.records);
            BM_LAUNCH_CHECK();
        }
    }
    if (!w4) {
        k_pack<<<blocks_for(n - 1, BLOCK), BLOCK, 0, s>>>(n, b.leaf_size, b.lch, b.rch, b.first, b.last, b.vals,
                                                         no_aabb, b.meshes, b.num_meshes, ob(b.ibox), ob(b.pre), ob(b.suf), ob(b.table), b.bounds,
                                                         rec2);
        BM_LAUNCH_CHECK();
    }
    return w8 ? launch_pack8(b, s) : hipSuccess;
}

constexpr uint32_t NRM_BLOCKS = 448;  // normal-gathering workgroups beside the top-digit pass's tiles (merged: 128 -> 0.260 ms, 256 -> 0.249, 448 -> 0.244)
constexpr uint32_t REC_DEFER_MAX_N = 1u << 19;  // bunny 0.068 -> 0.067 ms, armadillo 0.100 -> 0.099; merged 0.244 -> 0.250

bool msd_sort(uint32_t n, const Tuning& t) {
    static_assert(MSD_MAX_N <= MSD_MAX_N_CAP, "the LSD fallback inside k_bucket_sort covers at most RADIX tiles");
    return (int64_t)n <= std::min<int64_t>(t.get(BM_PARAM_MSD_MAX_N, MSD_MAX_N), MSD_MAX_N_CAP) && n >= MSD_MIN_N;
}
uint32_t build_sort_skew_word() { return META_SORT_SKEW; }

hipError_t launch_build(const BuildBuffers& b, hipStream_t s) {
    const uint32_t n = b.n;
    hipError_t e;
    // bounds, sort tickets, digit histograms and look-back words all start at zero: the gather's own
    // words here (unless the previous build of this buffer cleared them), the rest by k_gather itself
    if (!(n && b.replicas_clean) &&
        (e = hipMemsetD32Async((hipDeviceptr_t)b.bounds, 0, n ? META_GATHER_CLEAR : build_meta_words(n), s)) !=
            hipSuccess)
        return e;
    if (n == 0) return launch_empty(b, s);
    static const Tuning dflt;
    const Tuning& tune = b.tune ? *b.tune : dflt;
    const bool msd = msd_sort(n, tune);
    // top-digit-first sorts: the triangle records and corner normals ride on the top-digit pass
    // (BM_PARAM_NRM_DEFER 0: in the gather)
    const bool nrm_defer = tune.get(BM_PARAM_NRM_DEFER, 1) != 0;
    const bool defer = msd && nrm_defer;
    const bool orig = need_orig(b);
    if (b.orig_written) *b.orig_written = orig;
    // the records too up to REC_DEFER_MAX_N triangles (above, the pass's extra workgroups outlast its
    // tiles), when this build writes them at all
    const bool defer_tri = defer && orig && n <= REC_DEFER_MAX_N;
    launch_gather_kernel(b, s,
                         G_BOUNDS | G_CEN | (orig && !defer_tri ? G_TRI : 0) | (!defer ? G_NRM : 0) |
                             (need_aabb(b) ? G_AABB : 0),
                         META_GATHER_CLEAR, (uint32_t)plan_offset(n));
    BM_LAUNCH_CHECK();
    // an odd number of passes: start in the scratch pair so the sorted data ends in keys/vals
    k_morton<<<blocks_for(n, SORT_TILE), MORTON_BLOCK, 0, s>>>(n, b.cen, b.bounds, b.keys2, b.vals2);
    BM_LAUNCH_CHECK();
    if (msd) {  // top digit (keys2 -> keys), then each bucket in place; or the LSD fallback (skew)
        // 256-lane bucket workgroups up to 2^19 keys at most (their fallback tiles must not outnumber the
        // top-digit pass's, whose count sizes the look-back area); the parameter can only lower that
        const bool wide = (int64_t)n > std::min<int64_t>(tune.get(BM_PARAM_MSD_WIDE_N, MSD_WIDE_N), MSD_WIDE_N);
        // buckets above this take the LSD fallback: the kernel's LDS capacity, or below it
        // BM_PARAM_BUCKET_LDS_CAP (tests force the fallback with 0)
        const uint32_t cap = (uint32_t)std::min<int64_t>(tune.get(BM_PARAM_BUCKET_LDS_CAP, 0xFFFFFFFFll),
                                                         (wide ? 1024 : 256) * BS_ITEMS);
        const RecJob rj{b.meshes, b.num_meshes, n, defer ? std::min<uint32_t>(NRM_BLOCKS, blocks_for(n, OS_BLOCK_N)) : 0u,
                        defer_tri ? b.tri_orig : nullptr, b.nrm};
        uint32_t* smeta = b.bounds + META_COUNTERS;
        uint32_t* plan = b.bounds + plan_offset(n);
        const uint32_t nb = onesweep_tiles(n);
        const int wi = onesweep_items(n);
        launch_onesweep(b.keys2, b.vals2, b.keys, b.vals, n, RADIX_PASSES - 1, RADIX_PASSES, smeta, s, rj, cap + 1, plan);
        BM_LAUNCH_CHECK();
        if (wide)
            k_bucket_sort<1024><<<RADIX, 1024, 0, s>>>(b.keys, b.vals, b.keys2, b.vals2, b.bounds, plan, n, nb, wi);
        else
            k_bucket_sort<256><<<RADIX, 256, 0, s>>>(b.keys, b.vals, b.keys2, b.vals2, b.bounds, plan, n, nb, wi);
        BM_LAUNCH_CHECK();
        return launch_finish(b, s);
    }
    uint32_t *ki = b.keys2, *vi = b.vals2, *ko = b.keys, *vo = b.vals;
    static_assert(RADIX_PASSES % 2 == 1, "sorted output must land in keys/vals");
    for (int pass = 0; pass < RADIX_PASSES; ++pass) {
        launch_onesweep(ki, vi, ko, vo, n, pass, RADIX_PASSES, b.bounds + META_COUNTERS, s);
        BM_LAUNCH_CHECK();
        uint32_t* tk = ki; ki = ko; ko = tk;
        uint32_t* tv = vi; vi = vo; vo = tv;
    }
    // sorted data is in b.keys / b.vals: tree, boxes and sorted triangle records in one pass
    return launch_finish(b, s);
}

#ifdef BM_BUILD_DIAG
hipError_t build_diag(unsigned long long* out) { return bdiag_io((const void*)&g_bdiag, out, 0, 9); }
#endif

hipError_t launch_gather(const BuildBuffers& b, hipStream_t s) {  // reference modes: no scene bounds needed
    if (b.n == 0) return hipSuccess;
    // zeroes bounds words 0-2 and the map after them: the reference-mode build's queue count, overflow
    // flag, top-bit count and top-bit map (KdBuild::qcount, topcount, topmap)
    launch_gather_kernel(b, s, G_TRI | G_NRM | G_AABB, 0, 3 + KD_TOPMAP_WORDS);
    BM_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_orig_records(const BuildBuffers& b, hipStream_t s) {  // tri_orig only (no boxes, normals, bounds)
    if (b.n == 0) return hipSuccess;
    launch_gather_kernel(b, s, G_TRI);
    BM_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys2, uint32_t* vals2, uint32_t n,
                             int key_bits, uint32_t* smeta, hipStream_t s, bool* in_scratch, bool meta_zeroed,
                             const uint32_t* topmap) {
    if (topmap && key_bits != 31) return hipErrorInvalidValue;  // the ranked top digit is bits 20-30
    const int passes = topmap ? 3 : (key_bits + RADIX_BITS - 1) / RADIX_BITS;
    if (passes < 1 || passes > 4) return hipErrorInvalidValue;
    hipError_t e;
    if (!meta_zeroed &&
        (e = hipMemsetD32Async((hipDeviceptr_t)smeta, 0, sort_meta_words(n, key_bits), s)) != hipSuccess)
        return e;
    *in_scratch = false;
    if (n == 0) return hipSuccess;
    k_digit_hist<<<blocks_for(n, DH_TILE), BLOCK, 0, s>>>(keys, n, passes, smeta, topmap);
    BM_LAUNCH_CHECK();
    uint32_t *ki = keys, *vi = vals, *ko = keys2, *vo = vals2;
    for (int pass = 0; pass < passes; ++pass) {
        launch_onesweep(ki, vi, ko, vo, n, pass, passes, smeta, s, RecJob{}, 0, nullptr,
                        topmap && pass == 2 ? topmap : nullptr);
        BM_LAUNCH_CHECK();
        uint32_t* tk = ki; ki = ko; ko = tk;
        uint32_t* tv = vi; vi = vo; vo = tv;
    }
    *in_scratch = (passes % 2) == 1;
    return hipSuccess;
}

hipError_t launch_radix_tree(const uint32_t* keys, uint32_t n, uint32_t* lch, uint32_t* rch, uint32_t* first,
                             uint32_t* last, uint32_t* parent_leaf, uint32_t* parent_int, hipStream_t s,
                             const uint32_t* n_dev) {
    if (n < 2) return hipSuccess;
    k_emit_lds<<<blocks_for(n - 1, EMIT_LDS_BLOCK), EMIT_LDS_BLOCK, 0, s>>>((int)n, keys, lch, rch, first, last,
                                                                          parent_leaf, parent_int, n_dev);
    BM_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_refit(const BuildBuffers& b, hipStream_t s) {
    const uint32_t n = b.n;
    hipError_t e;
    if (!(n && b.replicas_clean) && (e = hipMemsetD32Async((hipDeviceptr_t)b.bounds, 0, META_GATHER_CLEAR, s)) != hipSuccess)
        return e;
    if (n == 0) return launch_empty(b, s);
    const bool orig = need_orig(b);
    if (b.orig_written) *b.orig_written = orig;
    launch_gather_kernel(b, s, G_BOUNDS | G_NRM | (orig ? G_TRI : 0) | (need_aabb(b) ? G_AABB : 0));
    BM_LAUNCH_CHECK();
    return launch_finish(b, s);
}

}  // namespace bm
