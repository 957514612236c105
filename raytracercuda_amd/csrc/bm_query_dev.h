// bm_query_dev.h — device pieces the batch queries share beyond the ray quads of bm_trace_quad.h: the
// point-to-triangle function, the pruning bound and the node step of the distance-ordered traversal
// (bm_points.hip, bm_points_multi.hip), the nearest-triangle traversal itself (quad_nearest: bm_points.hip,
// bm_signed.hip), and the sorted per-query list in LDS with its quad-wide insert
// (bm_multihit.hip, bm_points_multi.hip). Each piece stands here as its first user wrote it.
#pragma once
#include "bm_trace_quad.h"

namespace bm {
namespace {

__device__ __forceinline__ bool finite3(const vec3f a) {
    return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff();
}

// ---- the nearest-triangle traversal -----------------------------------------------

// The closest point of one 48-B triangle record (v0 | id, e1, e2) to p: Ericson's seven regions (vertex
// v0, vertex v1, edge v0v1, vertex v2, edge v0v2, edge v1v2, interior; the first match wins) in float32,
// one rounding per operation in the order written (include/beam_c.h states it; the tests restate it). dd
// is the squared distance, (u, v) the barycentrics in the hit-attribute convention: the point is
// v0*(1-(u+v)) + v1*u + v2*v. The regions are chosen by selects in reverse order, so a later (earlier
// listed) match overrides; every region that divides does so once, through num / den. Where that
// division is 0/0 or 1/0 (a zero-area triangle outside its vertex regions) dd is NaN and never a candidate.
__device__ __forceinline__ void tri_nearest(const float4 a, const float4 b, const float4 cc, const vec3f p, float& dd,
                                            float& u, float& v) {
    const vec3f e1 = v3(b.x, b.y, b.z), e2 = v3(cc.x, cc.y, cc.z);
    const vec3f ap = sub(p, v3(a.x, a.y, a.z));
    const float d1 = dot(e1, ap), d2 = dot(e2, ap);
    const float a11 = dot(e1, e1), a12 = dot(e1, e2), a22 = dot(e2, e2);
    const float d3 = d1 - a11, d4 = d2 - a12, d5 = d1 - a12, d6 = d2 - a22;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float s = d4 - d3, r = d5 - d6;
    int reg = 7;
    float num = 1.0f, den = (va + vb) + vc;
    if (va <= 0.0f && s >= 0.0f && r >= 0.0f) reg = 6, num = s, den = s + r;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) reg = 5, num = d2, den = d2 - d6;
    if (d6 >= 0.0f && d5 <= d6) reg = 4;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) reg = 3, num = d1, den = d1 - d3;
    if (d3 >= 0.0f && d4 <= d3) reg = 2;
    if (d1 <= 0.0f && d2 <= 0.0f) reg = 1;
    const float w = num / den;
    u = reg == 2 ? 1.0f : reg == 3 ? w : reg == 6 ? 1.0f - w : reg == 7 ? vb * w : 0.0f;
    v = reg == 4 ? 1.0f : (reg == 5 || reg == 6) ? w : reg == 7 ? vc * w : 0.0f;
    const vec3f q = v3(ap.x - (e1.x * u + e2.x * v), ap.y - (e1.y * u + e2.y * v), ap.z - (e1.z * u + e2.z * v));
    dd = dot(q, q);
}

// The pruning bound for a best squared distance: (sqrt(best) + m)^2, never below best itself (its own
// rounding could otherwise land an ulp under a huge rmax^2). m absorbs what rounding can put a triangle's
// dd below the squared distance to a box that contains the triangle.
__device__ __forceinline__ float widen(float best, float m) {
    const float s = sqrtf(best) + m;
    return fmaxf(s * s, best);
}

// Node step of the nearest-triangle traversal: lane c loads child c of the 128-B record as quad_visit
// does and takes the squared distance from pt to its box (per axis max(lo - p, p - hi, 0), squared,
// summed in dot order). A child within `bound` is kept; the kept ones are ranked by order_key(boxdd, c)
// with quad_visit's DPP exchange, ranks 1..nh-1 pushed farthest first with boxdd as their stack key, the
// nearest returned to all four lanes (EMPTY_REF when none is kept). An empty slot (EMPTY_REF; its NaN
// box would read as distance 0 through fmaxf) is never kept.
template <typename QS>
__device__ __forceinline__ uint32_t nearest_visit(const TraceParams& p, uint32_t node, int c, const vec3f pt,
                                                  float bound, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const float lx = u2f(nd[0]), ly = u2f(nd[4]), lz = u2f(nd[8]);
    const float hx = u2f(nd[12]), hy = u2f(nd[16]), hz = u2f(nd[20]);
    const uint32_t ref = nd[24];
    const float dx = fmaxf(fmaxf(lx - pt.x, pt.x - hx), 0.0f);
    const float dy = fmaxf(fmaxf(ly - pt.y, pt.y - hy), 0.0f);
    const float dz = fmaxf(fmaxf(lz - pt.z, pt.z - hz), 0.0f);
    const float boxdd = (dx * dx + dy * dy) + dz * dz;
    const bool h = (ref != EMPTY_REF) & (boxdd <= bound);
    const uint32_t key = h ? order_key(boxdd, (uint32_t)c) : ~0u;
    const uint32_t k1 = dpp_u<QP_X1>(key), k2 = dpp_u<QP_X2>(key), k3 = dpp_u<QP_X3>(key);
    const uint32_t rank = (uint32_t)(k1 < key) + (uint32_t)(k2 < key) + (uint32_t)(k3 < key);
    uint32_t nh = h ? 4u : rank;  // a dropped child's key ~0u ranks after every kept one: its rank is their count
    nh = min(nh, dpp_u<QP_X1>(nh));
    nh = min(nh, dpp_u<QP_X2>(nh));
    if (h && rank > 0) st.put(sp + (int)(nh - 1u - rank), ref, boxdd);
    sp += max((int)nh - 1, 0);
    uint32_t nx = (h && rank == 0) ? ref : EMPTY_REF;
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

// Nearest triangle of one point over the quad: the lexicographic minimum of (dd, id) over the triangles
// with dd <= best on entry (rmax^2). One iteration is quad_closest's: the pending leaf, the pop that
// follows it, the node visit. The bound moves only when best improves: a handful of times per query.
// maxsp (COUNT): the most stack entries held at once.
template <bool COUNT, uint32_t PRIO, typename QS>
__device__ __forceinline__ void quad_nearest(const TraceParams& p, const QS& st, int c, const vec3f pt, float m,
                                             float& best, uint32_t& ibest, float& bu, float& bv,
                                             unsigned long long& cn, unsigned long long& ct, int& maxsp) {
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    uint32_t iter = 0;
    float bound = widen(best, m);
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, cnt = ((next >> 27) & 15u) + 1u;
            bool better = false;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                const uint32_t k = first + k0 + c;
                float dd = __builtin_inff(), u = 0.f, v = 0.f;
                uint32_t id = NO_TRI;
                if (k0 + c < cnt) {
                    const float4 a = p.tris[3 * k + 0], b = p.tris[3 * k + 1], cc = p.tris[3 * k + 2];
                    float d, uu, vv;
                    tri_nearest(a, b, cc, pt, d, uu, vv);
                    if (d == d) dd = d, u = uu, v = vv, id = f2u(a.w);  // NaN: never a candidate
                }
                quad_min_hit(dd, id, u, v);
                if (dd < best || (dd == best && id < ibest)) {
                    best = dd;
                    ibest = id;
                    bu = u;
                    bv = v;
                    better = true;
                }
            }
            if (better) bound = widen(best, m);
            if (COUNT && c == 0) ct += cnt;
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
}

// ---- the sorted per-query list ----------------------------------------------------

constexpr int MULTI_CAP_SMALL = 4, MULTI_CAP_LARGE = BM_MULTI_MAX_HITS;
static_assert(MULTI_CAP_LARGE == 16, "the list layout rotates within 16 slots of 16 bytes");
// waves per SIMD the registers must allow. Small lists: the quad kernels' 7. Large lists: 12 KB of stack
// and 16 KB of list per workgroup make five workgroups per CU (160 KB), so the registers need no more.
constexpr int MULTI_WAVES_LARGE = 5;

constexpr int QP_ROT = 0x93;  // quad_perm [3,0,1,2]: lane c reads lane c - 1, lane 0 reads lane 3

template <int CTRL>
__device__ __forceinline__ float4 dpp_f4(const float4 e) {
    return make_float4(dpp_f<CTRL>(e.x), dpp_f<CTRL>(e.y), dpp_f<CTRL>(e.z), dpp_f<CTRL>(e.w));
}

__device__ __forceinline__ uint32_t quad_sum(uint32_t v) {
    v += dpp_u<QP_X1>(v);
    v += dpp_u<QP_X2>(v);
    return v;
}

// Lexicographic (t, id) minimum of the quad's candidates: quad_min_hit without the barycentrics, which stay
// with their owner lane until it writes the list entry.
template <int CTRL>
__device__ __forceinline__ void quad_min_tid_step(float& t, uint32_t& id) {
    const float ot = dpp_f<CTRL>(t);
    const uint32_t oid = dpp_u<CTRL>(id);
    const bool take = ot < t || (ot == t && oid < id);
    t = take ? ot : t;
    id = take ? oid : id;
}
__device__ __forceinline__ void quad_min_tid(float& t, uint32_t& id) {
    quad_min_tid_step<QP_X1>(t, id);
    quad_min_tid_step<QP_X2>(t, id);
}

// (t, id) order of two entries
__device__ __forceinline__ bool hit_below(float t, uint32_t id, float ot, uint32_t oid) {
    return t < ot || (t == ot && id < oid);
}

// Per-ray sorted list of a quad: LDS [ray][CAP] of 16-B entries (t, u, v, id bits: the bm_hit image),
// entry j of ray r in slot (j + 4r) mod CAP of r's row. ds_read_b128 serves a wave in four groups of four
// quads ({0,3,5,6}, {1,2,4,7} and the same + 8) over 16 slots of 16 B per bank row: with CAP = 16 the
// quad's lanes read slots 4(s + q) + c of their rows, with CAP = 4 slots 4q + c of the bank row — each
// group's 16 lanes on 16 different slots either way, and the 8-lane groups of ds_write_b128 (two adjacent
// quads, 8 slots per 128-B bank row) likewise. Unrotated, [ray][16] puts the four quads of a group on
// the same four slots and [k][ray] the four lanes of a quad on one: both four-way conflicts.
// BM_MULTI_LAYOUT (A/B builds, tools/multihit_bench.py): 1 = [k][ray], 2 = [ray][CAP] unrotated.
#ifndef BM_MULTI_LAYOUT
#define BM_MULTI_LAYOUT 0
#endif
template <int CAP>
struct HitList {
    float4* s;  // QRAYS * CAP entries
    int ray;
    __device__ __forceinline__ float4& at(uint32_t j) const {
#if BM_MULTI_LAYOUT == 1
        return s[j * QRAYS + (uint32_t)ray];
#elif BM_MULTI_LAYOUT == 2
        return s[(uint32_t)ray * CAP + j];
#else
        return s[(uint32_t)ray * CAP + ((j + 4u * (uint32_t)ray) & (uint32_t)(CAP - 1))];
#endif
    }
};

// Inserts the quad's candidate (t, id) — every lane holds the pair, the lane `owner` also its u, v — into
// the list of cnt (<= k) entries, dropping the last entry of a full list; a candidate at or beyond
// position k changes nothing. The owner writes the new entry, lane j mod 4 the shifted entry j. tlast: the
// t of entry k - 1 once the list is full.
template <int CAP>
__device__ __forceinline__ void list_insert(const HitList<CAP>& hl, int c, uint32_t k, uint32_t& cnt, float t,
                                            uint32_t id, bool owner, float u, float v, float& tlast) {
    constexpr int STEPS = CAP / 4;
    const float4 none = make_float4(__builtin_inff(), 0.f, 0.f, u2f(NO_TRI));
    float4 e[STEPS];
    uint32_t below = 0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint32_t j = (uint32_t)c + 4u * s;
        e[s] = none;
        if (j < cnt) {
            e[s] = hl.at(j);
            below += hit_below(e[s].x, f2u(e[s].w), t, id) ? 1u : 0u;
        }
    }
    const uint32_t pos = quad_sum(below);
    if (pos >= k) return;
    const uint32_t ncnt = min(cnt + 1u, k);
    float4 carry = none;
    float lt = pos + 1u == k ? t : -__builtin_inff();
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint32_t j = (uint32_t)c + 4u * s;
        const float4 left = dpp_f4<QP_ROT>(e[s]);
        // old[j - 1]; selected per component (a select of whole float4s goes through private memory)
        const float4 prev = make_float4(c == 0 ? carry.x : left.x, c == 0 ? carry.y : left.y, c == 0 ? carry.z : left.z,
                                        c == 0 ? carry.w : left.w);
        carry = left;
        if (j > pos && j < ncnt) {
            hl.at(j) = prev;
            if (j + 1u == k) lt = prev.x;  // entry k - 1 is the new one or a shifted one: pos < k
        }
    }
    if (owner) hl.at(pos) = make_float4(t, u, v, u2f(id));
    cnt = ncnt;
    if (ncnt == k) {
        lt = fmaxf(lt, dpp_f<QP_X1>(lt));
        tlast = fmaxf(lt, dpp_f<QP_X2>(lt));
    }
}

}  // namespace
}  // namespace bm
