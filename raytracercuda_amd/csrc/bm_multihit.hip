// bm_multihit.hip — multi-hit ray queries: the k nearest hits of each ray of a caller's batch, in
// (t, id) order, and the number of crossings within tmax (bm_scene_trace_rays_multi). The third ray
// query beside closest and any hit: the same BVH4 traversal over ray quads (quad_visit, tri_test, the
// per-ray stack in LDS with the global overflow area behind it; bm_trace_quad.h unchanged), keeping a
// sorted list per ray where quad_closest keeps one best hit.
//   k_query_multi  persistent grid; a wave takes batches of 16 consecutive rays, lane 4q+c works for
//                  ray 16b+q — the shape of k_query_rays
// The list holds bm_hit images (t, u, v, id bits) in LDS beside the stack, [ray][CAP] with a ray's
// entries rotated by four slots per ray (HitList). Lane c of the quad owns entries j = c, c + 4, ...: an
// insert reads them once, counts the entries below the candidate (summed over the quad by DPP), and
// rewrites those behind the new position as old[j - 1] — the left neighbour's entry of the same step (a
// quad rotation by DPP), for lane 0 lane 3's entry of the step before; the candidate's owner lane writes
// the new entry. ceil(k / 4) steps per insert.
// Pruning: the bound is tmax until the list is full, then the last entry's t (count-all: always tmax);
// quad_visit takes it as its tmax and the pop skips entries beyond it, both inclusive, so a triangle
// tying the last entry's t with a lower id is still found. With k = 1 and no count-all the per-ray
// sequence of node visits, leaf tests and pops is quad_closest's (the tests compare the counters).
#include "bm_query_dev.h"

namespace bm {
namespace {

// The k nearest hits of one ray over the quad, and with ALL the number of accepted triangles. One
// iteration is quad_closest's: the pending leaf, the pop that follows it, the node visit(s).
// cnt: entries in the list on return; total (ALL): |H|, the same in every lane of the quad.
// FILTER (calls with filter flags; fray: the ray's index in the batch): a triangle accepted within the bound — the
// list's for a pruned query, tmax when everything is counted — is also put to filter_accept
// (bm_trace_quad.h); a rejected one is no candidate and is not counted. Off, the code is the unfiltered one.
template <bool COUNT, uint32_t PRIO, bool ALL, int CAP, bool FILTER, typename QS>
__device__ __forceinline__ void quad_multi(const TraceParams& p, const QS& st, const HitList<CAP>& hl, int c, uint32_t k,
                                           const vec3f o, const vec3f dir, const vec3f inv, float tmax, uint32_t& cnt,
                                           uint32_t& total, unsigned long long& cn, unsigned long long& ct,
                                           uint32_t fray = 0) {
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    if (COUNT && !p.num_tris && c == 0) ++cn;  // an empty scene: the all-empty root record, as quad_closest counts it
    uint32_t iter = 0, mine = 0;
    float tlast = -__builtin_inff();  // k = 0: the list is full from the start and takes nothing
    float bound = tmax;               // the traversal's: tmax, or the last entry's t once a pruned list is full
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, lcnt = ((next >> 27) & 15u) + 1u;
            for (uint32_t k0 = 0; k0 < lcnt; k0 += 4) {
                const uint32_t ti = first + k0 + c;
                float t = __builtin_inff(), u = 0.f, v = 0.f;
                uint32_t id = NO_TRI;
                if (k0 + c < lcnt) {
                    const float4 a = p.tris[3 * ti + 0], b = p.tris[3 * ti + 1], cc = p.tris[3 * ti + 2];
                    float tt, uu, vv;
                    bool acc = tri_test(a, b, cc, o, dir, tt, uu, vv) && tt > 0.0f && tt < 3.40282347e+38f && tt <= tmax;
                    if constexpr (FILTER)
                        acc = acc && (ALL || tt <= (cnt == k ? tlast : tmax)) &&
                              filter_accept<true>(p, fray, ti, f2u(a.w), dir, tt);
                    if (acc) {
                        t = tt;
                        id = f2u(a.w);
                        u = uu;
                        v = vv;
                        if (ALL) ++mine;
                    }
                }
                // beyond a full list's last entry: no place in it (a tie in t is decided by the insert)
                if (!(t <= (cnt == k ? tlast : tmax))) {
                    t = __builtin_inff();
                    id = NO_TRI;
                }
                for (;;) {  // the group's candidates in (t, id) order
                    float mt = t;
                    uint32_t mi = id;
                    quad_min_tid(mt, mi);
                    if (!(mt < __builtin_inff())) break;
                    const bool owner = id == mi;
                    list_insert<CAP>(hl, c, k, cnt, mt, mi, owner, u, v, tlast);
                    if (owner) {
                        t = __builtin_inff();
                        id = NO_TRI;
                    }
                }
            }
            if (!ALL && cnt == k) bound = tlast;
            if (COUNT && c == 0) ct += lcnt;
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            bool found = false;
            while (sp > 0) {
                --sp;
                uint32_t ref;
                float tt;
                st.get(sp, ref, tt);
                if (!(tt > bound)) {
                    next = ref;
                    found = true;
                    break;
                }
            }
            if (!found) break;
            if (next & LEAF_BIT) continue;  // a popped leaf: tested at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = quad_visit(p, next, c, o, inv, bound, true, st, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = quad_visit(p, next, c, o, inv, bound, true, st, sp);
        }
    }
    if (ALL) total = quad_sum(mine);
}

// Ray records as in k_query_rays; an invalid ray (closest mode's rule) is finished without traversal: k
// miss records, count 0. Lane c stores records j = c, c + 4, ... of its ray's k contiguous records
// straight from the list (16-B stores), the miss record beyond the list's end.
// FILTER: as in k_query_rays.
template <bool COUNT, uint32_t PRIO, bool ALL, int CAP, bool FILTER>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : CAP > MULTI_CAP_SMALL ? MULTI_WAVES_LARGE
                                                                                                       : QUAD_WAVES))) void
k_query_multi(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    __shared__ float4 s_list[QRAYS * CAP];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    HitList<CAP> hl;
    hl.s = s_list;
    hl.ray = w * 16 + q;
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    const uint32_t n = p.q_n, k = min(p.q_k, (uint32_t)CAP);
    float4* out = reinterpret_cast<float4*>(p.q_out);
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[2 * (size_t)sidx], r1 = p.q_rays[2 * (size_t)sidx + 1];
        const vec3f o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
        const float tmax = r0.w;
        bool valid = finite3(o) && finite3(d) && tmax > 0.0f;  // false for NaN
        if (FILTER && (p.q_flags & BM_RAYS_PAD_TMIN)) valid = valid && r1.w >= 0.0f && r1.w < __builtin_inff();
        __builtin_amdgcn_s_setprio(0);
        uint32_t cnt = 0, total = 0;
        if (valid) {
            const vec3f inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
            quad_multi<COUNT, PRIO, ALL, CAP, FILTER>(p, st, hl, c, k, o, d, inv, tmax, cnt, total, cn, ct, sidx);
            if (COUNT && c == 0) ch += ALL ? total : cnt;
        }
        const size_t base = (size_t)sidx * k;
#pragma unroll
        for (int s = 0; s < CAP / 4; ++s) {
            const uint32_t j = (uint32_t)c + 4u * s;
            if (j < k) {
                float4 rec = make_float4(__builtin_inff(), 0.f, 0.f, u2f(NO_TRI));
                if (j < cnt) rec = hl.at(j);
                out[base + j] = rec;
            }
        }
        if (c == 0 && p.q_counts) p.q_counts[sidx] = ALL ? total : cnt;
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
}

template <bool ALL, int CAP, bool FILTER>
void launch_prio(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_query_multi<true, 1, ALL, CAP, FILTER>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_query_multi<false, 0, ALL, CAP, FILTER>, p, s, nullptr);
    else launch_persistent(k_query_multi<false, 1, ALL, CAP, FILTER>, p, s, nullptr);
}

template <bool ALL, int CAP>
void launch_count(const TraceParams& p, bool count, hipStream_t s) {
    if (p.q_flags) launch_prio<ALL, CAP, true>(p, count, s);
    else launch_prio<ALL, CAP, false>(p, count, s);
}

}  // namespace

hipError_t launch_query_multi(const TraceParams& p, bool count_all, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || p.q_k > BM_MULTI_MAX_HITS || (p.q_k == 0 && !count_all) || (count_all && !p.q_counts))
        return hipErrorInvalidValue;
    if ((p.q_flags & BM_RAYS_PAD_MASK) && p.q_ent_n && !p.q_ent) return hipErrorInvalidValue;
    const bool large = p.q_k > (uint32_t)MULTI_CAP_SMALL;
    if (count_all) {
        if (large) launch_count<true, MULTI_CAP_LARGE>(p, count, s);
        else launch_count<true, MULTI_CAP_SMALL>(p, count, s);
    } else {
        if (large) launch_count<false, MULTI_CAP_LARGE>(p, count, s);
        else launch_count<false, MULTI_CAP_SMALL>(p, count, s);
    }
    return hipGetLastError();
}

}  // namespace bm
