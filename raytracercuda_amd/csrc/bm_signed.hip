// bm_signed.hip — signed-distance and occupancy queries: for each point of a caller's batch in device
// memory, whether it lies inside the scene's surface and, in distance mode, the closest-point record with
// that sign on its distance (bm_scene_signed_distances).
//   k_signed_points  persistent grid; a wave takes batches of 16 consecutive points (256 contiguous
//                    bytes), lane 4q+c works for point 16b+q — the shape of k_closest_points
// The nearest phase (distance mode) is the closest-point traversal as it stands (quad_nearest,
// bm_query_dev.h): the record is bm_scene_closest_points' bit for bit. The parity phase is the sign: for each
// of the one or three fixed sample directions D_j (BM_SIGNED_D*, include/beam_c.h) the parity of the number of
// ALL triangles the ray (p, D_j, +inf) crosses — the count bm_scene_trace_rays_multi gives with k = 0 and
// BM_MULTI_COUNT_ALL, & 1. Nothing is ordered and no list is kept: lane c slab-tests child c with the ray
// query's box test at bound +inf (so the leaves reached are the multi-hit query's), the kept children go on
// the stack in child order without a ranking exchange, the stack key is never read, and at a leaf lane c
// toggles one bit per accepted triangle; quad_sum at the end gives the parity. The kernel runs the parity
// phase first: then only the vote count is live across the nearest traversal, which is the phase short of
// registers.
#include "bm_query_dev.h"

namespace bm {
namespace {

// Node step of the parity traversal: quad_visit's box test on child c at tmax = +inf, then the kept
// children in child order — the lowest kept slot is returned to all four lanes (EMPTY_REF when none is
// kept), the others pushed so that they pop in slot order. A kept child's place is the number of kept
// slots below it, read from the quad's 4-bit kept mask (two DPP exchanges; quad_visit's ranking takes
// three and three compares).
template <typename QS>
__device__ __forceinline__ uint32_t parity_visit(const TraceParams& p, uint32_t node, int c, const vec3f o,
                                                 const vec3f inv, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const f32x2 bx = {u2f(nd[0]), u2f(nd[12])}, by = {u2f(nd[4]), u2f(nd[16])}, bz = {u2f(nd[8]), u2f(nd[20])};
    const uint32_t ref = nd[24];
    const f32x2 tx = (bx - f32x2{o.x, o.x}) * f32x2{inv.x, inv.x};
    const f32x2 ty = (by - f32x2{o.y, o.y}) * f32x2{inv.y, inv.y};
    const f32x2 tz = (bz - f32x2{o.z, o.z}) * f32x2{inv.z, inv.z};
    const float tn = fmaxf(fmaxf(fminf(tx.x, tx.y), fminf(ty.x, ty.y)), fminf(tz.x, tz.y));
    const float tf = fminf(fminf(fmaxf(tx.x, tx.y), fmaxf(ty.x, ty.y)), fmaxf(tz.x, tz.y));
    const bool h = (tn <= tf) & (tf >= 0.0f) & (tn <= __builtin_inff());
    uint32_t kept = h ? 1u << c : 0u;
    kept |= dpp_u<QP_X1>(kept);
    kept |= dpp_u<QP_X2>(kept);
    const int nh = __builtin_popcount(kept);
    const int rank = __builtin_popcount(kept & ((1u << c) - 1u));
    if (h && rank > 0) st.put(sp + (nh - 1 - rank), ref, 0.0f);
    sp += max(nh - 1, 0);
    uint32_t nx = (h && rank == 0) ? ref : EMPTY_REF;
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

// C & 1 of one point and one direction over the quad: C counts the triangles tri_test accepts for the ray
// (o, dir) with 0 < t < FLT_MAX, over every leaf whose boxes the ray enters. One iteration is
// quad_closest's: the pending leaf, the pop that follows it, the node visit(s). Every pop is taken.
template <bool COUNT, uint32_t PRIO, typename QS>
__device__ __forceinline__ uint32_t quad_parity(const TraceParams& p, const QS& st, int c, const vec3f o,
                                                const vec3f dir, const vec3f inv, unsigned long long& cn,
                                                unsigned long long& ct) {
    int sp = 0;
    uint32_t next = 0, iter = 0, mine = 0;
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, lcnt = ((next >> 27) & 15u) + 1u;
            for (uint32_t k0 = 0; k0 < lcnt; k0 += 4) {
                const uint32_t ti = first + k0 + c;
                if (k0 + c < lcnt) {
                    float tt, uu, vv;
                    if (tri_test(p.tris[3 * ti + 0], p.tris[3 * ti + 1], p.tris[3 * ti + 2], o, dir, tt, uu, vv) &&
                        tt > 0.0f && tt < 3.40282347e+38f)
                        mine ^= 1u;
                }
            }
            if (COUNT && c == 0) ct += lcnt;
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            if (sp == 0) break;
            --sp;
            float key;
            st.get(sp, next, key);
            if (next & LEAF_BIT) continue;  // a popped leaf: tested at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = parity_visit(p, next, c, o, inv, st, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = parity_visit(p, next, c, o, inv, st, sp);
        }
    }
    return quad_sum(mine) & 1u;
}

// Component k of sample direction j (BM_SIGNED_D*, include/beam_c.h: D0 = (a, b, c), D1 = (-b, c, a),
// D2 = (c, -a, b)). The direction loop stays rolled (unrolled, the distance kernel with three votes spills
// at six waves): j is wave-uniform, so a direction and its reciprocal are literals chosen by scalar selects.
// The reciprocal is the IEEE quotient the multi-hit kernel computes for the same ray record.
constexpr float signed_dir(int j, int k) {
    constexpr float a = BM_SIGNED_DA, b = BM_SIGNED_DB, c = BM_SIGNED_DC;
    return j == 0 ? (k == 0 ? a : k == 1 ? b : c) : j == 1 ? (k == 0 ? -b : k == 1 ? c : a) : (k == 0 ? c : k == 1 ? -a : b);
}

// waves per SIMD the registers must allow: the most without scratch — 7 with one vote (72 and 66 VGPRs), 6 with
// three, where the rolled direction loop's state spills 2 to 3 VGPRs at 7
constexpr int SIGNED_WAVES = QUAD_WAVES, SIGNED_WAVES_VOTE3 = 6;

// A point record is one float4 (p, rmax); the four lanes of a quad load the same 16 bytes. An invalid
// point (a non-finite component of p; in distance mode also rmax NaN or <= 0) is finished here as outside
// with the miss record, so no NaN reaches a traversal. The scene scale of the nearest phase's pruning margin is
// k_closest_points'. The votes travel in p.q_counts (a byte per point; null: none wanted).
template <bool COUNT, uint32_t PRIO, uint32_t MODE, bool VOTE3>
__global__ __launch_bounds__(BLOCK)
__attribute__((amdgpu_waves_per_eu(COUNT ? 1 : VOTE3 ? SIGNED_WAVES_VOTE3 : SIGNED_WAVES))) void
k_signed_points(const TraceParams p) {
    constexpr bool DIST = MODE == BM_SIGNED_DISTANCE;
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, pn = 0, pt = 0;
    const unsigned long long none[3] = {0, 0, 0};
    int maxsp = 0;
    float root = 0.0f;  // the largest |coordinate| of the root's child boxes (empty slots are NaN: fmaxf skips them)
    if (DIST && p.num_tris) {
        const uint4* rn = p.nodes;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint4 pl = rn[k];
            root = fmaxf(root, fmaxf(fmaxf(fabsf(u2f(pl.x)), fabsf(u2f(pl.y))), fmaxf(fabsf(u2f(pl.z)), fabsf(u2f(pl.w)))));
        }
    }
    uint8_t* votes = reinterpret_cast<uint8_t*>(p.q_counts);
    const uint32_t n = p.q_n;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[sidx];
        const vec3f pt3 = v3(r0.x, r0.y, r0.z);
        const float rmax = r0.w;
        const bool valid = finite3(pt3) && (!DIST || rmax > 0.0f);  // false for NaN
        __builtin_amdgcn_s_setprio(0);
        float best = __builtin_inff(), bu = 0.f, bv = 0.f;
        uint32_t ibest = NO_TRI, sum = 0;
        if (valid && p.num_tris) {
#pragma unroll 1
            for (int j = 0; j < (VOTE3 ? 3 : 1); ++j) {
                const vec3f d = v3(signed_dir(j, 0), signed_dir(j, 1), signed_dir(j, 2));
                sum += quad_parity<COUNT, PRIO>(p, st, c, pt3, d, v3(1.f / d.x, 1.f / d.y, 1.f / d.z), pn, pt);
                if (PRIO) __builtin_amdgcn_s_setprio(0);
            }
            if (DIST) {  // after the parity rays: only their vote count is live across the nearest traversal
                best = rmax * rmax;
                const float m = 0x1p-18f * (fmaxf(fmaxf(fabsf(pt3.x), fabsf(pt3.y)), fabsf(pt3.z)) + root);
                quad_nearest<COUNT, PRIO>(p, st, c, pt3, m, best, ibest, bu, bv, cn, ct, maxsp);
            }
        }
        const bool inside = VOTE3 ? sum >= 2u : sum != 0u;
        if (c == 0) {
            if (DIST) {
                const float t = ibest == NO_TRI ? __builtin_inff() : sqrtf(best);
                // the result record: one 16-B store by the quad's first lane, as k_closest_points; the sign bit of t
                reinterpret_cast<float4*>(p.q_out)[sidx] =
                    make_float4(u2f(f2u(t) | (inside ? 0x80000000u : 0u)), bu, bv, u2f(ibest));
            } else {
                reinterpret_cast<uint8_t*>(p.q_out)[sidx] = inside ? 1 : 0;
            }
            if (votes) votes[sidx] = (uint8_t)sum;
        }
    }
    flush_counters<COUNT>(p, cn, ct, pn, none);
    if (COUNT) atomicAdd(&p.counters[3], pt);
}

template <uint32_t MODE, bool VOTE3>
void launch_mode(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_signed_points<true, 1, MODE, VOTE3>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_signed_points<false, 0, MODE, VOTE3>, p, s, nullptr);
    else launch_persistent(k_signed_points<false, 1, MODE, VOTE3>, p, s, nullptr);
}

}  // namespace

hipError_t launch_signed_points(const TraceParams& p, uint32_t mode, bool vote3, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_SIGNED_OCCUPANCY) return hipErrorInvalidValue;
    if (mode == BM_SIGNED_DISTANCE) {
        if (vote3) launch_mode<BM_SIGNED_DISTANCE, true>(p, count, s);
        else launch_mode<BM_SIGNED_DISTANCE, false>(p, count, s);
    } else {
        if (vote3) launch_mode<BM_SIGNED_OCCUPANCY, true>(p, count, s);
        else launch_mode<BM_SIGNED_OCCUPANCY, false>(p, count, s);
    }
    return hipGetLastError();
}

}  // namespace bm
