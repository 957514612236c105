// bm_normals.hip — smooth vertex normals of a deforming mesh (bm_mesh_compute_normals): the mesh's normal slot
// rewritten from its position slot and its indices, on the context stream, with a result defined to the bit.
//   k_vertex_normals  one pass, one lane per vertex. The lane walks its row of the vertex -> corner table (a CSR
//                     the host built once per index buffer: offsets[nv + 1], then the corner ids 3f + k stably
//                     sorted by vertex, so a row lists its corners in ascending order). Per corner it loads the
//                     face's index triple and the three positions and forms the face vector itself: no
//                     intermediate face-vector array, one launch. The row's first load depends on the offsets,
//                     the triple on the corner id, the positions on the triple: three dependent loads per
//                     corner, all L2-resident at the sizes this runs at, and neighbouring lanes' rows are
//                     neighbouring runs of the corner array.
// Arithmetic (include/beam_c.h, compared bit for bit): float32, one rounding per operation, no contraction:
//   e1 = p[i1] - p[i0], e2 = p[i2] - p[i0];
//   face vector (e1.y*e2.z - e2.y*e1.z, e1.z*e2.x - e2.z*e1.x, e1.x*e2.y - e2.x*e1.y)  (BM_ATTR_GEOM_NORMAL's);
//   s = (0,0,0), then s += face vector per corner of the row, in ascending corner order;
//   NORMALIZE: d = (s.x*s.x + s.y*s.y) + s.z*s.z; if d > 0, s *= 1.f / sqrtf(d)  (BM_ATTR_NORMALIZE's).
// The sum's order is the table's, so no atomic and no launch shape can touch a bit of the result.
// Nothing is read past the table's rows or written past the slot's nv vertices; a lane at or past nv does nothing.
#include "bm_internal.h"

namespace bm {
namespace {

constexpr int NORMALS_BLOCK = 256;

// global address space, for global_load/store instead of flat accesses
typedef __attribute__((address_space(1))) const float cgf1;
typedef __attribute__((address_space(1))) float gf1;
typedef __attribute__((address_space(1))) const uint32_t cgu1;

template <bool NORMALIZE>
__global__ __launch_bounds__(NORMALS_BLOCK) void k_vertex_normals(const float* __restrict__ pos_,
                                                                  const uint32_t* __restrict__ idx_,
                                                                  const uint32_t* __restrict__ offsets_,
                                                                  const uint32_t* __restrict__ corners_,
                                                                  float* __restrict__ nrm_, uint32_t nv) {
    const uint32_t v = blockIdx.x * NORMALS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    cgf1* pos = (cgf1*)pos_;
    cgu1* idx = (cgu1*)idx_;
    cgu1* offsets = (cgu1*)offsets_;
    cgu1* corners = (cgu1*)corners_;
    gf1* nrm = (gf1*)nrm_;
    const uint32_t c0 = offsets[v], c1 = offsets[v + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (uint32_t c = c0; c < c1; ++c) {
        const size_t f3 = 3 * (size_t)(corners[c] / 3u);
        const size_t i0 = 3 * (size_t)idx[f3], i1 = 3 * (size_t)idx[f3 + 1], i2 = 3 * (size_t)idx[f3 + 2];
        const float ax = pos[i0], ay = pos[i0 + 1], az = pos[i0 + 2];
        const float e1x = pos[i1] - ax, e1y = pos[i1 + 1] - ay, e1z = pos[i1 + 2] - az;
        const float e2x = pos[i2] - ax, e2y = pos[i2 + 1] - ay, e2z = pos[i2 + 2] - az;
        sx = sx + (e1y * e2z - e2y * e1z);
        sy = sy + (e1z * e2x - e2z * e1x);
        sz = sz + (e1x * e2y - e2x * e1y);
    }
    if constexpr (NORMALIZE) {
        const float d = (sx * sx + sy * sy) + sz * sz;
        if (d > 0.f) {
            const float il = 1.f / sqrtf(d);
            sx = sx * il, sy = sy * il, sz = sz * il;
        }
    }
    const size_t o = 3 * (size_t)v;
    nrm[o] = sx, nrm[o + 1] = sy, nrm[o + 2] = sz;
}

}  // namespace

hipError_t launch_vertex_normals(const float* pos, const uint32_t* idx, const uint32_t* offsets,
                                 const uint32_t* corners, float* nrm, uint32_t nv, bool normalize, hipStream_t s) {
    if (nv == 0) return hipSuccess;
    const uint32_t grid = (nv + NORMALS_BLOCK - 1) / NORMALS_BLOCK;
    if (normalize) k_vertex_normals<true><<<grid, NORMALS_BLOCK, 0, s>>>(pos, idx, offsets, corners, nrm, nv);
    else k_vertex_normals<false><<<grid, NORMALS_BLOCK, 0, s>>>(pos, idx, offsets, corners, nrm, nv);
    return hipGetLastError();
}

}  // namespace bm
