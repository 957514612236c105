// bm_xform.hip — instance transforms: the scene-owned, world-space copies of an instanced mesh's positions
// and normals (bm_scene_add_instance), written before every build and refit of a scene that has instances.
//   k_instance_xform  one launch for all instance entries. A work unit is one wave over XFORM_UNIT (256)
//                     consecutive vertices of one entry; the host laid the units' prefix per entry. The wave
//                     finds its entry by a wave-uniform binary search over the packed prefix (skipped for a
//                     single entry), so the row's pointers and 21 matrix floats are scalar loads. A lane takes
//                     4 vertices = 48 bytes: three 16-byte loads and stores per array (regions start on
//                     16-byte boundaries: the host aligned the pool regions, hipMalloc the sources). The
//                     last nv % 4 vertices of an entry go one float at a time.
// Arithmetic (include/beam_c.h, compared bit for bit): float32, one rounding per operation, no contraction:
//   position  x' = ((x[0]*px + x[1]*py) + x[2]*pz) + x[3], rows 1 and 2 alike;
//   normal    n' = (c[3r]*nx + c[3r+1]*ny) + c[3r+2]*nz with c = bm_xform_normal_matrix(x), from the host.
// Nothing is read or written past an entry's nv vertices; a unit at or past num_units does nothing.
#include "bm_internal.h"

namespace bm {
namespace {

constexpr int XFORM_BLOCK = 256;  // four waves, one unit each

// The row's pointers come out of memory, so the compiler cannot tell their address space: global here, for
// global_load/store_dwordx4 instead of flat accesses.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gf4;
typedef __attribute__((address_space(1))) float gf1;

__device__ __forceinline__ void xform_pos(const float* __restrict__ x, float px, float py, float pz, float& ox,
                                          float& oy, float& oz) {
    ox = ((x[0] * px + x[1] * py) + x[2] * pz) + x[3];
    oy = ((x[4] * px + x[5] * py) + x[6] * pz) + x[7];
    oz = ((x[8] * px + x[9] * py) + x[10] * pz) + x[11];
}

__device__ __forceinline__ void xform_nrm(const float* __restrict__ c, float nx, float ny, float nz, float& ox,
                                          float& oy, float& oz) {
    ox = (c[0] * nx + c[1] * ny) + c[2] * nz;
    oy = (c[3] * nx + c[4] * ny) + c[5] * nz;
    oz = (c[6] * nx + c[7] * ny) + c[8] * nz;
}

// Four vertices (12 floats at a 16-byte aligned address) through one of the two maps.
template <bool POS>
__device__ __forceinline__ void xform4(const float* __restrict__ m, const float* __restrict__ src,
                                       float* __restrict__ dst) {
    const gf4* s4 = (const gf4*)src;
    const f32x4 a = s4[0], b = s4[1], c = s4[2];
    const float in[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    float out[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if constexpr (POS) xform_pos(m, in[3 * k], in[3 * k + 1], in[3 * k + 2], out[3 * k], out[3 * k + 1], out[3 * k + 2]);
        else xform_nrm(m, in[3 * k], in[3 * k + 1], in[3 * k + 2], out[3 * k], out[3 * k + 1], out[3 * k + 2]);
    }
    gf4* d4 = (gf4*)dst;
    d4[0] = f32x4{out[0], out[1], out[2], out[3]};
    d4[1] = f32x4{out[4], out[5], out[6], out[7]};
    d4[2] = f32x4{out[8], out[9], out[10], out[11]};
}

__global__ __launch_bounds__(XFORM_BLOCK) void k_instance_xform(const XformRow* __restrict__ rows,
                                                                const uint32_t* __restrict__ prefix,
                                                                uint32_t num_entries, uint32_t num_units) {
    const uint32_t unit = __builtin_amdgcn_readfirstlane(blockIdx.x * (XFORM_BLOCK / 64) + (threadIdx.x >> 6));
    if (unit >= num_units) return;
    uint32_t e = 0;
    if (num_entries > 1) {
        // the last entry whose first unit is <= unit; prefix[0] = 0, and an entry without units repeats its
        // successor's value and is stepped over
        uint32_t hi = num_entries;
        while (hi - e > 1) {
            const uint32_t mid = e + ((hi - e) >> 1);
            if (prefix[mid] <= unit) e = mid;
            else hi = mid;
        }
        e = __builtin_amdgcn_readfirstlane(e);
    }
    const XformRow& r = rows[e];
    const uint32_t nv = r.nv;
    const uint32_t v0 = (unit - r.unit_first) * XFORM_UNIT + (threadIdx.x & 63u) * 4u;
    if (v0 >= nv) return;
    const size_t f0 = 3 * (size_t)v0;
    if (nv - v0 >= 4) {
        xform4<true>(r.x, r.src_pos + f0, r.dst_pos + f0);
        xform4<false>(r.c, r.src_nrm + f0, r.dst_nrm + f0);
    } else {
        const gf1* sp = (const gf1*)r.src_pos;
        const gf1* sn = (const gf1*)r.src_nrm;
        gf1* dp = (gf1*)r.dst_pos;
        gf1* dn = (gf1*)r.dst_nrm;
        for (uint32_t k = 0; k < nv - v0; ++k) {
            const size_t f = f0 + 3 * (size_t)k;
            float ox, oy, oz;
            xform_pos(r.x, sp[f], sp[f + 1], sp[f + 2], ox, oy, oz);
            dp[f] = ox, dp[f + 1] = oy, dp[f + 2] = oz;
            xform_nrm(r.c, sn[f], sn[f + 1], sn[f + 2], ox, oy, oz);
            dn[f] = ox, dn[f + 1] = oy, dn[f + 2] = oz;
        }
    }
}

}  // namespace

hipError_t launch_instance_xform(const XformRow* rows, const uint32_t* prefix, uint32_t num_entries,
                                 uint32_t num_units, hipStream_t s) {
    if (num_entries == 0 || num_units == 0) return hipSuccess;
    const uint32_t per_block = XFORM_BLOCK / 64;
    const uint32_t grid = (uint32_t)(((uint64_t)num_units + per_block - 1) / per_block);
    k_instance_xform<<<grid, XFORM_BLOCK, 0, s>>>(rows, prefix, num_entries, num_units);
    return hipGetLastError();
}

}  // namespace bm
