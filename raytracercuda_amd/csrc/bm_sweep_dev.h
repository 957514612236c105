// bm_sweep_dev.h — device pieces of the sphere-cast query (bm_sweep.hip): the swept-sphere function of one
// triangle record, the pruning margin and the node step of its traversal.
#pragma once
#include "bm_query_dev.h"

namespace bm {
namespace {

// The smaller root of qa t^2 + 2 qb t + qc against the infinite cylinder of squared radius rr around the
// line P + s E, for the centre line m + t d (m = origin - P): accepted when the discriminant is >= 0, the
// leading coefficient > 0, the foot parameter s within [0, 1] and 0 <= t <= tl. dd = dot(d,d), md =
// dot(m,d), mm = dot(m,m). One rounding per operation in the order written (include/beam_c.h states it).
__device__ __forceinline__ bool sweep_edge(const vec3f m, const vec3f E, const vec3f d, float dd, float md, float mm,
                                           float rr, float tl, float& t, float& s) {
    const float EE = dot(E, E), Ed = dot(E, d), Em = dot(E, m);
    const float qa = EE * dd - Ed * Ed;
    const float qb = EE * md - Ed * Em;
    const float qc = EE * (mm - rr) - Em * Em;
    const float disc = qb * qb - qa * qc;
    t = (-qb - sqrtf(disc)) / qa;
    s = (Em + t * Ed) / EE;
    return disc >= 0.0f && qa > 0.0f && s >= 0.0f && s <= 1.0f && t >= 0.0f && t <= tl;
}

// The smaller root against the sphere of squared radius rr around P: accepted when the discriminant is
// >= 0, dd > 0 and 0 <= t <= tl.
__device__ __forceinline__ bool sweep_vertex(float dd, float md, float mm, float rr, float tl, float& t) {
    const float disc = md * md - dd * (mm - rr);
    t = (-md - sqrtf(disc)) / dd;
    return disc >= 0.0f && dd > 0.0f && t >= 0.0f && t <= tl;
}

// First contact of the sphere of radius r whose centre moves as o + t d, 0 <= t <= tl, with one 48-B
// triangle record (v0 | id, e1, e2). Start: tri_nearest(o) within r*r gives t = 0 with tri_nearest's (u, v).
// Otherwise seven candidates in this order — the face (the centre's line against the plane offset by r
// towards the origin's side, accepted when the sphere moves towards the plane and the contact's
// barycentrics lie in the triangle), the edges v0v1, v0v2, v1v2 (sweep_edge), the vertices v0, v1, v2
// (sweep_vertex) — and the smallest accepted t wins, the earlier candidate on equal t (strict <). (u, v)
// are the contact point's barycentrics in the hit-attribute convention. A NaN is never accepted: every
// acceptance is a chain of comparisons that are false for NaN.
__device__ __forceinline__ bool tri_sweep(const float4 a, const float4 b, const float4 cc, const vec3f o, const vec3f d,
                                          float r, float tl, float& t, float& u, float& v) {
    const vec3f e1 = v3(b.x, b.y, b.z), e2 = v3(cc.x, cc.y, cc.z);
    float dd0, u0, v0;
    tri_nearest(a, b, cc, o, dd0, u0, v0);
    const float rr = r * r;
    const vec3f ap = sub(o, v3(a.x, a.y, a.z));
    const float dd = dot(d, d);
    float tb = __builtin_inff(), ub = 0.0f, vb = 0.0f;
    {  // 1. the face
        const vec3f n = cross(e1, e2);
        const float nn = dot(n, n), h = dot(n, ap), nd = dot(n, d);
        const float ln = sqrtf(nn);
        const float hs = fabsf(h), nds = h >= 0.0f ? nd : -nd;  // |n| x: the distance to the plane, the approach speed
        const float tf = (hs - r * ln) / (-nds);
        const vec3f w = v3(ap.x + d.x * tf, ap.y + d.y * tf, ap.z + d.z * tf);
        const float fu = dot(n, cross(w, e2)) / nn, fv = dot(n, cross(e1, w)) / nn;
        if (nds < 0.0f && fu >= 0.0f && fv >= 0.0f && fu + fv <= 1.0f && tf >= 0.0f && tf <= tl) tb = tf, ub = fu, vb = fv;
    }
    const float md0 = dot(ap, d), mm0 = dot(ap, ap);
    const vec3f m1 = sub(ap, e1), m2 = sub(ap, e2);
    const float md1 = dot(m1, d), mm1 = dot(m1, m1);
    const float md2 = dot(m2, d), mm2 = dot(m2, m2);
    float tc, s;
    if (sweep_edge(ap, e1, d, dd, md0, mm0, rr, tl, tc, s) && tc < tb) tb = tc, ub = s, vb = 0.0f;       // 2. v0 -> v1
    if (sweep_edge(ap, e2, d, dd, md0, mm0, rr, tl, tc, s) && tc < tb) tb = tc, ub = 0.0f, vb = s;       // 3. v0 -> v2
    if (sweep_edge(m1, sub(e2, e1), d, dd, md1, mm1, rr, tl, tc, s) && tc < tb) tb = tc, ub = 1.0f - s, vb = s;  // 4. v1 -> v2
    if (sweep_vertex(dd, md0, mm0, rr, tl, tc) && tc < tb) tb = tc, ub = 0.0f, vb = 0.0f;               // 5. v0
    if (sweep_vertex(dd, md1, mm1, rr, tl, tc) && tc < tb) tb = tc, ub = 1.0f, vb = 0.0f;               // 6. v1
    if (sweep_vertex(dd, md2, mm2, rr, tl, tc) && tc < tb) tb = tc, ub = 0.0f, vb = 1.0f;               // 7. v2
    const bool start = dd0 <= rr;  // false for NaN
    t = start ? 0.0f : tb;
    u = start ? u0 : ub;
    v = start ? v0 : vb;
    return start || tb < __builtin_inff();
}

// The pruning margin of one sweep: rel is the largest |origin - vertex| component the scene
// allows (against the union of the root's child boxes), big the largest |coordinate| of the origin plus that
// of the boxes. Whenever tri_sweep accepts a t, the centre o + t d lies within r + m/2 of the triangle (m/17
// measured); the rest of m covers the padded planes' and the slab products' own rounding.
__device__ __forceinline__ float sweep_margin(float rel, float r, float big) {
    return 0x1p-7f * (rel + r) + 0x1p-16f * big;
}

// Node step of the sweep traversal: lane c loads child c of the 128-B record as quad_visit does, moves its
// planes outwards by pad (= r + m, one rounding each) and slab-tests the centre's line against that box:
// t = (plane - o) * inv per plane, quad_visit's formulation. A child with tn <= tf, tf >= 0 and tn <= bound
// is kept; the kept ones are ranked by order_key(tn, c) with quad_visit's DPP exchange, ranks 1..nh-1 pushed
// farthest first with tn as their stack key, the nearest returned to all four lanes (EMPTY_REF when none is
// kept). An empty slot (EMPTY_REF, an all-NaN box) is never kept.
template <typename QS>
__device__ __forceinline__ uint32_t sweep_visit(const TraceParams& p, uint32_t node, int c, const vec3f o,
                                                const vec3f inv, float pad, float bound, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const float lx = u2f(nd[0]) - pad, ly = u2f(nd[4]) - pad, lz = u2f(nd[8]) - pad;
    const float hx = u2f(nd[12]) + pad, hy = u2f(nd[16]) + pad, hz = u2f(nd[20]) + pad;
    const uint32_t ref = nd[24];
    const float x0 = (lx - o.x) * inv.x, x1 = (hx - o.x) * inv.x;
    const float y0 = (ly - o.y) * inv.y, y1 = (hy - o.y) * inv.y;
    const float z0 = (lz - o.z) * inv.z, z1 = (hz - o.z) * inv.z;
    const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    const bool h = (ref != EMPTY_REF) & (tn <= tf) & (tf >= 0.0f) & (tn <= bound);
    const uint32_t key = h ? order_key(tn, (uint32_t)c) : ~0u;
    const uint32_t k1 = dpp_u<QP_X1>(key), k2 = dpp_u<QP_X2>(key), k3 = dpp_u<QP_X3>(key);
    const uint32_t rank = (uint32_t)(k1 < key) + (uint32_t)(k2 < key) + (uint32_t)(k3 < key);
    uint32_t nh = h ? 4u : rank;  // a dropped child's key ~0u ranks after every kept one: its rank is their count
    nh = min(nh, dpp_u<QP_X1>(nh));
    nh = min(nh, dpp_u<QP_X2>(nh));
    if (h && rank > 0) st.put(sp + (int)(nh - 1u - rank), ref, tn);
    sp += max((int)nh - 1, 0);
    uint32_t nx = (h && rank == 0) ? ref : EMPTY_REF;
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

}  // namespace
}  // namespace bm
