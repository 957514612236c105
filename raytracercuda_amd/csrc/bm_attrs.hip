// bm_attrs.hip — hit attributes: the meshes' vertex slots interpolated at the hits of a ray query
// (bm_scene_hit_attributes). The reference's bmFaceInterpolate<T> (CudaComon.cuh:253-266) for any slot,
// in the operation order of shade_normals (bm_trace_dev.h, shared by every trace kernel): w = 1 - (u + v); (a0*w + a1*u) + a2*v.
//   k_hit_attrs<NREQ>  one lane per bm_hit record: a 16-B load of the record, the mesh by binary search
//                      over the packed tri_offset array (skipped for a one-mesh scene), the face's three
//                      indices, then per request three vertex reads and one row store. The mesh and the
//                      indices are found once and shared by the NREQ requests.
// A miss (tri_id at or above the built triangle count) reads nothing but its record: zero rows, all-ones
// for BM_ATTR_MESH_FACE. Only tri_id indexes memory; the host checked every mesh's largest index against
// its vertex count before the launch (bm_api.cpp).
#include "bm_internal.h"

namespace bm {
namespace {

constexpr int ATTR_BLOCK = 256;

template <int C>
__device__ __forceinline__ void load_vertex(const float* __restrict__ base, uint32_t i, float (&a)[C]) {
    const float* p = base + (size_t)i * C;
    if constexpr (C == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
    } else if constexpr (C == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        a[0] = q.x, a[1] = q.y;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = p[c];
    }
}

template <int C>
__device__ __forceinline__ void store_row(void* out, size_t i, const float (&r)[C]) {
    float* p = reinterpret_cast<float*>(out) + i * C;
    if constexpr (C == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else if constexpr (C == 2) *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
    else {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = r[c];
    }
}

__device__ __forceinline__ void normalize3(float (&r)[3]) {
    const float il = 1.f / sqrtf(dot(v3(r[0], r[1], r[2]), v3(r[0], r[1], r[2])));
    r[0] = r[0] * il, r[1] = r[1] * il, r[2] = r[2] * il;
}

// One request's row of hit i. base: the slot's buffer in the hit's mesh, null for a miss or a mesh
// without the slot (a zero row).
template <int C>
__device__ __forceinline__ void slot_row(const AttrReq& q, const float* __restrict__ base, size_t i, uint32_t i0,
                                         uint32_t i1, uint32_t i2, float u, float v, float w) {
    float r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = 0.f;
    if (base) {
        float a0[C], a1[C], a2[C];
        load_vertex<C>(base, i0, a0);
        load_vertex<C>(base, i1, a1);
        load_vertex<C>(base, i2, a2);
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = (a0[c] * w + a1[c] * u) + a2[c] * v;
        if constexpr (C == 3)
            if (q.normalize) normalize3(r);
    }
    store_row<C>(q.out, i, r);
}

__device__ __forceinline__ void geom_normal_row(const AttrReq& q, const float* __restrict__ pos, size_t i, uint32_t i0,
                                                uint32_t i1, uint32_t i2) {
    float r[3] = {0.f, 0.f, 0.f};
    if (pos) {
        float a0[3], a1[3], a2[3];
        load_vertex<3>(pos, i0, a0);
        load_vertex<3>(pos, i1, a1);
        load_vertex<3>(pos, i2, a2);
        const vec3f v0 = v3(a0[0], a0[1], a0[2]);
        const vec3f n = cross(sub(v3(a1[0], a1[1], a1[2]), v0), sub(v3(a2[0], a2[1], a2[2]), v0));
        r[0] = n.x, r[1] = n.y, r[2] = n.z;
        if (q.normalize) normalize3(r);
    }
    store_row<3>(q.out, i, r);
}

template <int NREQ>
__global__ __launch_bounds__(ATTR_BLOCK) void k_hit_attrs(const AttrParams p) {
    const size_t i = (size_t)blockIdx.x * ATTR_BLOCK + threadIdx.x;
    if (i >= p.n) return;
    const float4 h = p.hits[i];
    const uint32_t g = f2u(h.w);
    const bool hit = g < p.num_tris;
    uint32_t m = 0, f = 0, i0 = 0, i1 = 0, i2 = 0;
    const AttrMesh* __restrict__ md = nullptr;
    if (hit) {
        if (p.num_meshes > 1) {
            // the last mesh whose offset is <= g: meshes without triangles repeat their successor's offset
            // and are stepped over; offsets[0] = 0 <= g, so the invariant offsets[m] <= g holds from the start
            uint32_t hi = p.num_meshes;
            while (hi - m > 1) {
                const uint32_t mid = m + ((hi - m) >> 1);
                if (p.offsets[mid] <= g) m = mid;
                else hi = mid;
            }
        }
        md = p.meshes + m;
        f = g - md->tri_offset;
        const uint32_t* __restrict__ ix = md->idx + 3 * (size_t)f;
        i0 = ix[0], i1 = ix[1], i2 = ix[2];
    }
    const float u = h.y, v = h.z;
    const float w = 1.f - (u + v);
#pragma unroll
    for (int r = 0; r < NREQ; ++r) {
        const AttrReq& q = p.req[r];
        if (q.kind == ATTR_MESH_FACE) {
            reinterpret_cast<uint2*>(q.out)[i] = hit ? make_uint2(m, f) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        } else if (q.kind == ATTR_GEOM_NORMAL) {
            geom_normal_row(q, hit ? md->slot[BM_VERTEX_DATA_POSITION] : nullptr, i, i0, i1, i2);
        } else {
            const float* base = hit ? md->slot[q.slot] : nullptr;
            switch (q.comps) {  // wave-uniform
                case 1: slot_row<1>(q, base, i, i0, i1, i2, u, v, w); break;
                case 2: slot_row<2>(q, base, i, i0, i1, i2, u, v, w); break;
                case 3: slot_row<3>(q, base, i, i0, i1, i2, u, v, w); break;
                default: slot_row<4>(q, base, i, i0, i1, i2, u, v, w); break;
            }
        }
    }
}

}  // namespace

hipError_t launch_hit_attrs(const AttrParams& p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    if (p.num_reqs < 1 || p.num_reqs > BM_ATTR_MAX_REQS) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((uint64_t)p.n + ATTR_BLOCK - 1) / ATTR_BLOCK);
    switch (p.num_reqs) {
        case 1: k_hit_attrs<1><<<grid, ATTR_BLOCK, 0, s>>>(p); break;
        case 2: k_hit_attrs<2><<<grid, ATTR_BLOCK, 0, s>>>(p); break;
        case 3: k_hit_attrs<3><<<grid, ATTR_BLOCK, 0, s>>>(p); break;
        default: k_hit_attrs<4><<<grid, ATTR_BLOCK, 0, s>>>(p); break;
    }
    return hipGetLastError();
}

}  // namespace bm
