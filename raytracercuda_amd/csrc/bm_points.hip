// bm_points.hip — closest-point queries: for each point of a caller's batch in device memory, the nearest
// triangle of the scene, its distance and where on it (bm_scene_closest_points). The result is a bm_hit
// (distance, u, v, tri_id), so bm_scene_hit_attributes turns it into the closest point, the normal there
// or the owning mesh and face.
//   k_closest_points  persistent grid; a wave takes batches of 16 consecutive points (256 contiguous
//                     bytes), lane 4q+c works for point 16b+q — the shape of k_query_rays
// The traversal (quad_nearest, in bm_query_dev.h since bm_signed.hip shares it) is distance ordered over
// the BVH4: lane c takes child c's squared box
// distance, the kept children are ranked by order_key and pushed farthest first with that distance as
// their stack key, and a subtree is dropped when its box lies beyond a widened image of the best squared
// distance found so far. The widening makes the pruning conservative against the rounding of the
// triangle function, so the result is the lexicographic minimum of (dd, id) over ALL triangles, bit for
// bit what an exhaustive evaluation of tri_nearest gives.
#include "bm_query_dev.h"

namespace bm {
namespace {

// A point record is one float4 (p, rmax); the four lanes of a quad load the same 16 bytes. An invalid
// point (a non-finite component of p; rmax NaN or <= 0) is finished here with the miss record, so no NaN
// reaches the traversal. The scene scale of the pruning margin comes from the root record's child boxes
// (wave-uniform loads, once per kernel).
template <bool COUNT, uint32_t PRIO>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : QUAD_WAVES))) void
k_closest_points(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    int maxsp = 0;
    float root = 0.0f;  // the largest |coordinate| of the root's child boxes (empty slots are NaN: fmaxf skips them)
    if (p.num_tris) {
        const uint4* rn = p.nodes;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint4 pl = rn[k];
            root = fmaxf(root, fmaxf(fmaxf(fabsf(u2f(pl.x)), fabsf(u2f(pl.y))), fmaxf(fabsf(u2f(pl.z)), fabsf(u2f(pl.w)))));
        }
    }
    const uint32_t n = p.q_n;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[sidx];
        const vec3f pt = v3(r0.x, r0.y, r0.z);
        const float rmax = r0.w;
        const bool valid = finite3(pt) && rmax > 0.0f;  // false for NaN
        __builtin_amdgcn_s_setprio(0);
        float best = __builtin_inff(), bu = 0.f, bv = 0.f;
        uint32_t ibest = NO_TRI;
        if (valid) {
            best = rmax * rmax;
            const float m = 0x1p-18f * (fmaxf(fmaxf(fabsf(pt.x), fabsf(pt.y)), fabsf(pt.z)) + root);
            quad_nearest<COUNT, PRIO>(p, st, c, pt, m, best, ibest, bu, bv, cn, ct, maxsp);
            if (COUNT && c == 0 && ibest != NO_TRI) ++ch;
        }
        const float t = ibest == NO_TRI ? __builtin_inff() : sqrtf(best);
        // the result record: one 16-B store by the quad's first lane, as k_query_rays
        if (c == 0) reinterpret_cast<float4*>(p.q_out)[sidx] = make_float4(t, bu, bv, u2f(ibest));
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

}  // namespace

hipError_t launch_closest_points(const TraceParams& p, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4) return hipErrorInvalidValue;
    if (count) launch_persistent(k_closest_points<true, 1>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_closest_points<false, 0>, p, s, nullptr);
    else launch_persistent(k_closest_points<false, 1>, p, s, nullptr);
    return hipGetLastError();
}

}  // namespace bm
