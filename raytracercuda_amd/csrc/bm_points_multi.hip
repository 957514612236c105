// bm_points_multi.hip — multi-result point queries: for each point of a caller's batch the k nearest
// triangles within rmax in (dd, id) order, each with its closest point, and the number of triangles within
// rmax (bm_scene_closest_points_multi). The point side's counterpart of bm_multihit.hip: the distance-
// ordered traversal of bm_points.hip (nearest_visit, tri_nearest, the widened bound; bm_query_dev.h) keeping
// bm_multihit.hip's sorted list per query (HitList, list_insert) where quad_nearest keeps one best.
//   k_closest_points_multi  persistent grid; a wave takes batches of 16 consecutive points, lane 4q+c works
//                           for point 16b+q — the shape of k_closest_points and k_query_multi
// The list holds (dd, u, v, id bits): ordering and pruning use the squared distance, as the definition
// does, and sqrtf is applied once where a record is copied out.
// Pruning: the bound is widen(rmax^2, m) until the list is full, then widen(dd of the last entry, m)
// (count-all: always widen(rmax^2, m)), with §18's absolute margin m: the triangle function and the box
// distance are quad_nearest's, so its derivation holds for the k-th distance as for the first. The child
// test and the pop are inclusive, so a triangle tying the last entry's dd with a lower id is still
// reached. With k = 1 and no count-all the per-point sequence of node visits, leaf evaluations and pops is
// quad_nearest's (the tests compare the counters).
#include "bm_query_dev.h"

namespace bm {
namespace {

// The k nearest triangles of one point over the quad among those with dd <= lim (rmax^2), and with ALL
// their number. One iteration is quad_nearest's: the pending leaf, the pop that follows it, the node
// visit(s). cnt: entries in the list on return; total (ALL): |N|, the same in every lane of the quad;
// maxsp (COUNT): the most stack entries held at once.
template <bool COUNT, uint32_t PRIO, bool ALL, int CAP, typename QS>
__device__ __forceinline__ void quad_nearest_multi(const TraceParams& p, const QS& st, const HitList<CAP>& hl, int c,
                                                   uint32_t k, const vec3f pt, float m, float lim, uint32_t& cnt,
                                                   uint32_t& total, unsigned long long& cn, unsigned long long& ct,
                                                   int& maxsp) {
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    uint32_t iter = 0, mine = 0;
    float ddlast = -__builtin_inff();  // k = 0: the list is full from the start and takes nothing
    float bdd = lim;                   // what the bound was widened from: rmax^2, or a pruned full list's last dd
    float bound = widen(bdd, m);
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, lcnt = ((next >> 27) & 15u) + 1u;
            for (uint32_t k0 = 0; k0 < lcnt; k0 += 4) {
                const uint32_t ti = first + k0 + c;
                float dd = __builtin_inff(), u = 0.f, v = 0.f;
                uint32_t id = NO_TRI;
                if (k0 + c < lcnt) {
                    const float4 a = p.tris[3 * ti + 0], b = p.tris[3 * ti + 1], cc = p.tris[3 * ti + 2];
                    float d, uu, vv;
                    tri_nearest(a, b, cc, pt, d, uu, vv);
                    if (d <= lim) {  // NaN: never a candidate
                        dd = d;
                        id = f2u(a.w);
                        u = uu;
                        v = vv;
                        if (ALL) ++mine;
                    }
                }
                // beyond a full list's last entry: no place in it (a tie in dd is decided by the insert)
                if (!(dd <= (cnt == k ? ddlast : lim))) {
                    dd = __builtin_inff();
                    id = NO_TRI;
                }
                for (;;) {  // the group's candidates in (dd, id) order
                    float md = dd;
                    uint32_t mi = id;
                    quad_min_tid(md, mi);
                    if (mi == NO_TRI) break;  // by id: a dd of +inf within rmax = +inf is a candidate too
                    const bool owner = id == mi;
                    list_insert<CAP>(hl, c, k, cnt, md, mi, owner, u, v, ddlast);
                    if (owner) {
                        dd = __builtin_inff();
                        id = NO_TRI;
                    }
                }
            }
            if (!ALL && cnt == k && ddlast != bdd) {  // the last entry changed
                bdd = ddlast;
                bound = widen(bdd, m);
            }
            if (COUNT && c == 0) ct += lcnt;
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            bool found = false;
            while (sp > 0) {
                --sp;
                uint32_t ref;
                float key;
                st.get(sp, ref, key);
                if (!(key > bound)) {
                    next = ref;
                    found = true;
                    break;
                }
            }
            if (!found) break;
            if (next & LEAF_BIT) continue;  // a popped leaf: evaluated at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = nearest_visit(p, next, c, pt, bound, st, sp);
        if (COUNT) maxsp = max(maxsp, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = nearest_visit(p, next, c, pt, bound, st, sp);
            if (COUNT) maxsp = max(maxsp, sp);
        }
    }
    if (ALL) total = quad_sum(mine);
}

// Point records and the scene scale of the margin as in k_closest_points; an invalid point (its rule) is
// finished without traversal: k miss records, count 0. Lane c stores records j = c, c + 4, ... of its
// point's k contiguous records from the list (16-B stores) with t = sqrtf(dd), the miss record beyond the
// list's end.
template <bool COUNT, uint32_t PRIO, bool ALL, int CAP>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : CAP > MULTI_CAP_SMALL ? MULTI_WAVES_LARGE
                                                                                                       : QUAD_WAVES))) void
k_closest_points_multi(const TraceParams p) {
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
    int maxsp = 0;
    float root = 0.0f;  // the largest |coordinate| of the root's child boxes (empty slots are NaN: fmaxf skips them)
    if (p.num_tris) {
        const uint4* rn = p.nodes;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const uint4 pl = rn[i];
            root = fmaxf(root, fmaxf(fmaxf(fabsf(u2f(pl.x)), fabsf(u2f(pl.y))), fmaxf(fabsf(u2f(pl.z)), fabsf(u2f(pl.w)))));
        }
    }
    const uint32_t n = p.q_n, k = min(p.q_k, (uint32_t)CAP);
    float4* out = reinterpret_cast<float4*>(p.q_out);
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[sidx];
        const vec3f pt = v3(r0.x, r0.y, r0.z);
        const float rmax = r0.w;
        const bool valid = finite3(pt) && rmax > 0.0f;  // false for NaN
        __builtin_amdgcn_s_setprio(0);
        uint32_t cnt = 0, total = 0;
        if (valid) {
            const float m = 0x1p-18f * (fmaxf(fmaxf(fabsf(pt.x), fabsf(pt.y)), fabsf(pt.z)) + root);
            quad_nearest_multi<COUNT, PRIO, ALL, CAP>(p, st, hl, c, k, pt, m, rmax * rmax, cnt, total, cn, ct, maxsp);
            if (COUNT && c == 0) ch += ALL ? total : cnt;
        }
        const size_t base = (size_t)sidx * k;
#pragma unroll
        for (int s = 0; s < CAP / 4; ++s) {
            const uint32_t j = (uint32_t)c + 4u * s;
            if (j < k) {
                float4 rec = make_float4(__builtin_inff(), 0.f, 0.f, u2f(NO_TRI));
                if (j < cnt) {
                    rec = hl.at(j);
                    rec.x = sqrtf(rec.x);
                }
                out[base + j] = rec;
            }
        }
        if (c == 0 && p.q_counts) p.q_counts[sidx] = ALL ? total : cnt;
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

template <bool ALL, int CAP>
void launch_count(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_closest_points_multi<true, 1, ALL, CAP>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_closest_points_multi<false, 0, ALL, CAP>, p, s, nullptr);
    else launch_persistent(k_closest_points_multi<false, 1, ALL, CAP>, p, s, nullptr);
}

}  // namespace

hipError_t launch_closest_points_multi(const TraceParams& p, bool count_all, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || p.q_k > BM_MULTI_MAX_HITS || (p.q_k == 0 && !count_all) || (count_all && !p.q_counts))
        return hipErrorInvalidValue;
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
