// bm_rays.hip — ray queries: closest hit and any hit over a caller's batch of rays in device memory
// (bm_scene_trace_rays). The traversal is the quad kernels' own (quad_closest / quad_anyhit of
// bm_trace_quad.h, unchanged): four lanes per ray over the BVH4, the per-ray stack in LDS with the
// global overflow area behind it, so a query returns what a camera trace of the same rays returns
// and its COUNT build counts what oracle/beam_oracle.c counts.
//   k_query_rays  persistent grid; a wave takes batches of 16 consecutive rays (512 contiguous bytes
//                 of ray records), lane 4q+c works for ray 16b+q
// The rays are traced in the order given. An ordering pass (a 30-bit origin/direction key per ray,
// launch_sort_pairs, results scattered to the rays' own indices) was built and measured slower than
// that on the incoherent workloads it was meant for, and is not here.
#include "bm_trace_quad.h"

namespace bm {
namespace {

constexpr int RAYS_CLOSEST = BM_RAYS_CLOSEST, RAYS_ANY_HIT = BM_RAYS_ANY_HIT;

__device__ __forceinline__ bool finite3(const vec3f a) {
    return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff();
}

// A ray record is two float4: (origin, tmax) (dir, pad). The four lanes of a quad load the same 32
// bytes (one request per 16-B piece). An invalid ray (a non-finite origin or direction component;
// closest mode: tmax NaN or <= 0) is finished here without traversal, so no NaN reaches a traversal
// loop: the miss record, or 0. FILTER: the call has filter flags (p.q_flags); the traversal's filter reads the
// ray's pad word, and with BM_RAYS_PAD_TMIN a pad that is not a finite float >= 0 makes the ray
// invalid like the others.
template <int MODE, bool COUNT, uint32_t PRIO, bool FILTER>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : QUAD_WAVES))) void
k_query_rays(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    const uint32_t n = p.q_n;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[2 * (size_t)sidx], r1 = p.q_rays[2 * (size_t)sidx + 1];
        const vec3f o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
        bool valid = finite3(o) && finite3(d);
        if (FILTER && (p.q_flags & BM_RAYS_PAD_TMIN))
            valid = valid && r1.w >= 0.0f && r1.w < __builtin_inff();  // tmin: false for NaN
        __builtin_amdgcn_s_setprio(0);
        if (MODE == RAYS_CLOSEST) {
            const float tmax = r0.w;
            valid = valid && tmax > 0.0f;  // false for NaN
            float tbest = __builtin_inff(), bu = 0.f, bv = 0.f;
            uint32_t ibest = NO_TRI;
            if (valid) {
                const vec3f inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
                tbest = tmax;
                quad_closest<COUNT, PRIO, QStack<QUAD_LDS>, 4, FILTER>(p, st, c, o, d, inv, tbest, ibest, bu, bv, cn, ct,
                                                                       sidx);
                if (ibest == NO_TRI) tbest = __builtin_inff();
                else if (COUNT && c == 0) ++ch;
            }
            // the result record: one 16-B store by the quad's first lane (a dword per lane measured
            // alike: DESIGN.md §14)
            if (c == 0) reinterpret_cast<float4*>(p.q_out)[sidx] = make_float4(tbest, bu, bv, u2f(ibest));
        } else {
            bool occ = false;
            if (valid && p.num_tris) {  // quad_anyhit starts at the root without looking at num_tris
                occ = quad_anyhit<COUNT, PRIO, QStack<QUAD_LDS>, 4, FILTER>(p, st, c, o, d, cn, ct, sidx);
                if (COUNT && c == 0) ch += occ;
            }
            if (c == 0) reinterpret_cast<uint8_t*>(p.q_out)[sidx] = occ ? 1 : 0;
        }
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
}

template <int MODE, bool FILTER>
void launch_count(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_query_rays<MODE, true, 1, FILTER>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_query_rays<MODE, false, 0, FILTER>, p, s, nullptr);
    else launch_persistent(k_query_rays<MODE, false, 1, FILTER>, p, s, nullptr);
}

template <int MODE>
void launch_filter(const TraceParams& p, bool count, hipStream_t s) {
    if (p.q_flags) launch_count<MODE, true>(p, count, s);
    else launch_count<MODE, false>(p, count, s);
}

}  // namespace

hipError_t launch_query_rays(const TraceParams& p, uint32_t mode, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_RAYS_ANY_HIT) return hipErrorInvalidValue;
    if ((p.q_flags & BM_RAYS_PAD_MASK) && p.q_ent_n && !p.q_ent) return hipErrorInvalidValue;
    if (mode == BM_RAYS_CLOSEST) launch_filter<RAYS_CLOSEST>(p, count, s);
    else launch_filter<RAYS_ANY_HIT>(p, count, s);
    return hipGetLastError();
}

}  // namespace bm
