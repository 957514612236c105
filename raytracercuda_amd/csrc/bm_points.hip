// bm_points.hip — closest-point queries: for each point of a caller's batch in device memory, the nearest
// triangle of the scene, its distance and where on it (bm_scene_closest_points). The result is a bm_hit
// (distance, u, v, tri_id), so bm_scene_hit_attributes turns it into the closest point, the normal there
// or the owning mesh and face.
//   k_closest_points  persistent grid; a wave takes batches of 16 consecutive points (256 contiguous
//                     bytes), lane 4q+c works for point 16b+q — the shape of k_query_rays
// The traversal (quad_nearest) is distance ordered over the BVH4: lane c takes child c's squared box
// distance, the kept children are ranked by order_key and pushed farthest first with that distance as
// their stack key, and a subtree is dropped when its box lies beyond a widened image of the best squared
// distance found so far. The widening makes the pruning conservative against the rounding of the
// triangle function, so the result is the lexicographic minimum of (dd, id) over ALL triangles, bit for
// bit what an exhaustive evaluation of tri_nearest gives.
#include "bm_trace_quad.h"

namespace bm {
namespace {

__device__ __forceinline__ bool finite3(const vec3f a) {
    return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff();
}

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
