// bm_trace_quad.h — ray quads: four lanes per ray over the BVH4 (quad_closest, quad_anyhit), the
// persistent quad kernel and the compacted form (k_cull + k_trace_rays). Shared pieces: bm_trace_dev.h.
#pragma once
#include "bm_trace_dev.h"

namespace bm {
namespace {

// ---- ray quads: four lanes per ray over the BVH4 --------------------------------------------------
// A wave traces a 4x4 pixel tile: lane 4q+c works for ray q. At a node lane c slab-tests child c
// (one dword of each SoA plane: the quad's four loads hit one 16-B segment); at a leaf lane c tests
// triangles first+c, first+c+4, ... Ranks, the nearest child and the closest hit are combined
// across the quad with DPP quad permutations, so every lane of a quad holds the same ray state
// (next, sp, tbest, ibest, u, v) and the quad's control flow is uniform. Per ray a node step costs
// about a third of the single-lane step's instructions and a leaf of up to four triangles one
// triangle test, so the grazing rays that set the frame time (SURVEY §8(a) a4's hot loop, the
// critical path of the heaviest 8x8 tiles) finish in a fraction of the dependent steps. The
// traversal order (stable nearest-first child order, pop-skip of entries beyond tbest) and
// therefore the COUNT build's counters are exactly those of trace_pixel / orc_bvh_trace.
constexpr int QRAYS = BLOCK / 4;  // rays per workgroup
constexpr uint32_t LPT_MAX = 128;  // tiles of one workgroup's share the cost-ordered schedule sorts
// Cost-ordered scheduling needs every share (tiles b, b + B, ... in the XCD-aware order) to fit LPT_MAX.
__host__ __device__ __forceinline__ bool lpt_share_fits(uint32_t ntiles, uint32_t blocks) {
    return blocks >= 8 && (blocks & 7u) == 0 && (ntiles + blocks - 1) / blocks + 8 <= LPT_MAX;
}

constexpr int QUAD_WAVES = 7;  // waves per SIMD the quad kernels' registers must allow (72 VGPRs; 8 measured slower)
constexpr int QUAD_WAVES_FUSED = 7;  // with fused shadow rays (6 waves: 80 VGPRs, measured 6-10 % slower)
// Pixel tile of one wave of the quad kernel (16 rays): QTW x QTH. 4x4 writes each plane row as 16-B
// pieces that L2 merges only partly (WRITE_SIZE 1.58x the planes' bytes); 8x2 writes 32-B pieces
// (1.26x) but its rays are less coherent: 4-14 % slower.
constexpr uint32_t QTW = 4, QTH = 16 / QTW;
static_assert(QTW * QTH == 16, "a wave traces 16 rays");
constexpr int QUAD_LDS = 24;  // LDS stack entries per ray (>= the fallback's 12: the overflow area fits both)
// quad_closest: node visits per loop iteration while the nearest child is internal (3, 4: within 1 %
// in flight, single frame 1-2 % slower)
constexpr int QUAD_VISITS = 2;

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return i2f(__builtin_amdgcn_mov_dpp(f2i(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
constexpr int QP_X1 = 0xB1;  // quad_perm [1,0,3,2]: lane c reads lane c^1
constexpr int QP_X2 = 0x4E;  // quad_perm [2,3,0,1]: lane c^2
constexpr int QP_X3 = 0x1B;  // quad_perm [3,2,1,0]: lane c^3

// Lexicographic (t, id) minimum of the quad's candidates; u, v travel with the winner.
template <int CTRL>
__device__ __forceinline__ void quad_min_step(float& t, uint32_t& id, float& u, float& v) {
    const float ot = dpp_f<CTRL>(t), ou = dpp_f<CTRL>(u), ov = dpp_f<CTRL>(v);
    const uint32_t oid = dpp_u<CTRL>(id);
    const bool take = ot < t || (ot == t && oid < id);
    t = take ? ot : t;
    id = take ? oid : id;
    u = take ? ou : u;
    v = take ? ov : v;
}
__device__ __forceinline__ void quad_min_hit(float& t, uint32_t& id, float& u, float& v) {
    quad_min_step<QP_X1>(t, id, u, v);
    quad_min_step<QP_X2>(t, id, u, v);
}

// Per-ray stack of a quad: LDS [depth][ray] of (ref, t) pairs below LDS_N (one 8-B read or write
// per entry), the global overflow area beyond. All four lanes pop the same entry (an LDS
// broadcast); a push is written by the lane that owns the child.
template <int LDS_N, int RAYS = QRAYS>
struct QStack {
    uint2 (*s)[RAYS];
    int ray;
    uint32_t* g_ref;  // overflow area bases (wave-uniform: kept in SGPRs) ...
    float* g_t;
    uint32_t slot;    // ... and this ray's slot in them (one VGPR instead of two 64-bit pointers)
    uint32_t stride;
    __device__ __forceinline__ void put(int sp, uint32_t ref, float t) const {
        if (sp < LDS_N) {
            s[sp][ray] = make_uint2(ref, f2u(t));
        } else {
            g_ref[(size_t)(sp - LDS_N) * stride + slot] = ref;
            g_t[(size_t)(sp - LDS_N) * stride + slot] = t;
        }
    }
    // The overflow side reads through an opaque global load (ovf_load): with plain loads the
    // compiler merges the two sides into one flat load through a selected pointer, and a flat load
    // waits on vmcnt(0) and lgkmcnt(0) — every pop would wait for all of the wave's outstanding
    // global memory traffic instead of one LDS read.
    __device__ __forceinline__ void get(int sp, uint32_t& ref, float& t) const {
        if (sp < LDS_N) {
            const uint2 e = s[sp][ray];
            ref = e.x;
            t = u2f(e.y);
        } else {
            ref = ovf_load(&g_ref[(size_t)(sp - LDS_N) * stride + slot]);
            t = u2f(ovf_load(reinterpret_cast<const uint32_t*>(&g_t[(size_t)(sp - LDS_N) * stride + slot])));
        }
    }
};

// Quad node step: lane c slab-tests child c of the 128-B record against [.., tmax]; the hit
// children are ranked by their order keys (order_key: entry distance, then slot), ranks 1..nh-1
// pushed farthest first (rank r at sp + nh-1-r) with push_t(tn) as their stack key, and the rank-0
// child returned to all four lanes (EMPTY_REF when nothing is hit) — visit4's order exactly.
// VALU economy (the quad kernels are issue-bound): the record is addressed by a
// 32-bit offset from the node base (one shift), the lo/hi planes of an axis go through packed f32
// subtract/multiply (each element one IEEE operation, as in the scalar form), a rank is three
// unsigned compares of DPP-exchanged keys, and the quad's hit count is the minimum over the quad of
// (hit ? 4 : rank) — a missing child's key ~0u ranks after every hit, so its rank is the hit count.
template <typename QS>
__device__ __forceinline__ uint32_t quad_visit(const TraceParams& p, uint32_t node, int c,
                                               const vec3f o, const vec3f inv, float tmax, bool key_t, const QS& st,
                                               int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const f32x2 bx = {u2f(nd[0]), u2f(nd[12])}, by = {u2f(nd[4]), u2f(nd[16])}, bz = {u2f(nd[8]), u2f(nd[20])};
    const uint32_t ref = nd[24];
    const f32x2 tx = (bx - f32x2{o.x, o.x}) * f32x2{inv.x, inv.x};
    const f32x2 ty = (by - f32x2{o.y, o.y}) * f32x2{inv.y, inv.y};
    const f32x2 tz = (bz - f32x2{o.z, o.z}) * f32x2{inv.z, inv.z};
    const float tn = fmaxf(fmaxf(fminf(tx.x, tx.y), fminf(ty.x, ty.y)), fminf(tz.x, tz.y));
    const float tf = fminf(fminf(fmaxf(tx.x, tx.y), fmaxf(ty.x, ty.y)), fmaxf(tz.x, tz.y));
    const bool h = (tn <= tf) & (tf >= 0.0f) & (tn <= tmax);
    const uint32_t key = h ? order_key(tn, (uint32_t)c) : ~0u;
    const uint32_t k1 = dpp_u<QP_X1>(key), k2 = dpp_u<QP_X2>(key), k3 = dpp_u<QP_X3>(key);
    const uint32_t rank = (uint32_t)(k1 < key) + (uint32_t)(k2 < key) + (uint32_t)(k3 < key);
    uint32_t nh = h ? 4u : rank;
    nh = min(nh, dpp_u<QP_X1>(nh));
    nh = min(nh, dpp_u<QP_X2>(nh));
    if (h && rank > 0) st.put(sp + (int)(nh - 1u - rank), ref, key_t ? tn : 0.0f);
    sp += max((int)nh - 1, 0);
    uint32_t nx = (h && rank == 0) ? ref : EMPTY_REF;
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

// BVH8 quad node step (256-B records, oracle width 8): lane c holds children 2c and 2c+1 — adjacent
// dwords of every SoA plane, one 8-B load per plane, the two slabs in packed f32 — and ranks each
// among all eight by order_key8 (the three partners' two keys by DPP). Positions, hit count and the
// next child as in quad_visit.
__device__ __forceinline__ uint32_t order_key8(float tn, uint32_t slot) {
    const int32_t b = f2i(tn) > 0 ? f2i(tn) : 0;
    return ((uint32_t)b & ~7u) | slot;
}

template <typename QS>
__device__ __forceinline__ uint32_t quad_visit8(const TraceParams& p, uint32_t node, int c, const vec3f o,
                                                const vec3f inv, float tmax, bool key_t, const QS& st, int& sp) {
    const uint2* nd = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(p.nodes) + ((size_t)node << 8)) + c;
    const uint2 lxp = nd[0], lyp = nd[4], lzp = nd[8], hxp = nd[12], hyp = nd[16], hzp = nd[20], rp = nd[24];
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const f32x2 ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
    const f32x2 tlx = (f32x2{u2f(lxp.x), u2f(lxp.y)} - ox) * ix, thx = (f32x2{u2f(hxp.x), u2f(hxp.y)} - ox) * ix;
    const f32x2 tly = (f32x2{u2f(lyp.x), u2f(lyp.y)} - oy) * iy, thy = (f32x2{u2f(hyp.x), u2f(hyp.y)} - oy) * iy;
    const f32x2 tlz = (f32x2{u2f(lzp.x), u2f(lzp.y)} - oz) * iz, thz = (f32x2{u2f(hzp.x), u2f(hzp.y)} - oz) * iz;
    const float tna = fmaxf(fmaxf(fminf(tlx.x, thx.x), fminf(tly.x, thy.x)), fminf(tlz.x, thz.x));
    const float tfa = fminf(fminf(fmaxf(tlx.x, thx.x), fmaxf(tly.x, thy.x)), fmaxf(tlz.x, thz.x));
    const float tnb = fmaxf(fmaxf(fminf(tlx.y, thx.y), fminf(tly.y, thy.y)), fminf(tlz.y, thz.y));
    const float tfb = fminf(fminf(fmaxf(tlx.y, thx.y), fmaxf(tly.y, thy.y)), fmaxf(tlz.y, thz.y));
    const bool ha = (tna <= tfa) & (tfa >= 0.0f) & (tna <= tmax);
    const bool hb = (tnb <= tfb) & (tfb >= 0.0f) & (tnb <= tmax);
    const uint32_t ka = ha ? order_key8(tna, 2u * (uint32_t)c) : ~0u;
    const uint32_t kb = hb ? order_key8(tnb, 2u * (uint32_t)c + 1u) : ~0u;
    const uint32_t a1 = dpp_u<QP_X1>(ka), a2 = dpp_u<QP_X2>(ka), a3 = dpp_u<QP_X3>(ka);
    const uint32_t b1 = dpp_u<QP_X1>(kb), b2 = dpp_u<QP_X2>(kb), b3 = dpp_u<QP_X3>(kb);
    const uint32_t ra = (uint32_t)(kb < ka) + (uint32_t)(a1 < ka) + (uint32_t)(a2 < ka) + (uint32_t)(a3 < ka) +
                        (uint32_t)(b1 < ka) + (uint32_t)(b2 < ka) + (uint32_t)(b3 < ka);
    const uint32_t rb = (uint32_t)(ka < kb) + (uint32_t)(a1 < kb) + (uint32_t)(a2 < kb) + (uint32_t)(a3 < kb) +
                        (uint32_t)(b1 < kb) + (uint32_t)(b2 < kb) + (uint32_t)(b3 < kb);
    // hit count: a missing child's key ~0u ranks after every hit, so its rank is the hit count
    uint32_t nh = min(ha ? 8u : ra, hb ? 8u : rb);
    nh = min(nh, dpp_u<QP_X1>(nh));
    nh = min(nh, dpp_u<QP_X2>(nh));
    if (ha && ra > 0) st.put(sp + (int)(nh - 1u - ra), rp.x, key_t ? tna : 0.0f);
    if (hb && rb > 0) st.put(sp + (int)(nh - 1u - rb), rp.y, key_t ? tnb : 0.0f);
    sp += max((int)nh - 1, 0);
    uint32_t nx = (ha && ra == 0) ? rp.x : ((hb && rb == 0) ? rp.y : EMPTY_REF);
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

template <int BW, typename QS>
__device__ __forceinline__ uint32_t quad_visit_w(const TraceParams& p, uint32_t node, int c, const vec3f o,
                                                 const vec3f inv, float tmax, bool key_t, const QS& st, int& sp) {
    if constexpr (BW == 8) return quad_visit8(p, node, c, o, inv, tmax, key_t, st, sp);
    else return quad_visit(p, node, c, o, inv, tmax, key_t, st, sp);
}

// ---- ray query filters (beam_c.h BM_RAYS_CULL_* / BM_RAYS_PAD_*) -------------------
// The filter of a ray query: does the call accept the triangle at sorted index k, which the triangle
// function has just accepted at distance t within the traversal's current bound? It runs on such
// candidates only — a few per ray, not one per triangle test — so everything it needs beyond t is
// fetched or recomputed here and costs the traversal no register: the ray's pad word (read as the
// flags say) from record `ray` of the batch, the triangle's global id and, for the cull flags, its
// determinant from its own edges (tri_det: the triangle test's statements). The tests on the call's
// flags (p.q_flags, wave-uniform) are scalar branches. For BM_RAYS_PAD_MASK the owner of the id is
// found by a binary search over the first ids of the entries that own triangles (p.q_ent), addressed
// by 32-bit byte offsets from the wave-uniform base (at most 2^27 entries). A rejected candidate
// becomes the "no candidate" value before the quad reduction, so it never tightens a bound.
// ID_LIVE: the caller holds the triangle's global id (closest and multi-hit record it anyway; any hit does not).
template <bool ID_LIVE>
__device__ __forceinline__ bool filter_accept(const TraceParams& p, uint32_t ray, uint32_t k, uint32_t id_live,
                                              const vec3f dir, float t) {
    const uint32_t flags = p.q_flags;
    // any hit: the index goes through an empty asm, or the compiler finds the record's address in the kernel's
    // own load of the ray and keeps that 64-bit address in registers across the whole traversal (12 B of
    // scratch at 7 waves per SIMD). The other two kernels fit as they are, and the multi-hit one spills with it.
    if (!ID_LIVE) asm volatile("" : "+v"(ray));
    const uint32_t pad = reinterpret_cast<const uint32_t*>(p.q_rays)[8 * (size_t)ray + 7];
    bool ok = t > ((flags & BM_RAYS_PAD_TMIN) ? u2f(pad) : 0.0f);
    if (flags & (BM_RAYS_CULL_BACK | BM_RAYS_CULL_FRONT)) {
        const float det = tri_det(p.tris[3 * k + 1], p.tris[3 * k + 2], dir);
        ok = ok && ((flags & BM_RAYS_CULL_BACK) ? det > 0.0f : det < 0.0f);
    }
    if (flags & (BM_RAYS_PAD_SKIP_TRI | BM_RAYS_PAD_MASK)) {
        const uint32_t id = ID_LIVE ? id_live : f2u(p.tris[3 * k].w);
        if (flags & BM_RAYS_PAD_SKIP_TRI) {
            ok = ok && id != pad;
        } else if (ok) {
            const char* ent = reinterpret_cast<const char*>(p.q_ent);
            const uint32_t n = p.q_ent_n;
            uint32_t lo = 0, hi = n;  // the owner: the last entry whose first id is <= id, in [lo, hi)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (*reinterpret_cast<const uint32_t*>(ent + (mid << 2)) <= id) lo = mid;
                else hi = mid;
            }
            ok = n != 0 && (*reinterpret_cast<const uint32_t*>(ent + ((n + lo) << 2)) & pad) != 0;
        }
    }
    return ok;
}

// Closest hit of one ray over the quad (trace_pixel's loop): t > 0, ties to the lowest id.
// FILTER (ray queries with filter flags; fray: the ray's index in the batch): a candidate is also put to
// filter_accept. Off, the code is the unfiltered one.
template <bool COUNT, uint32_t PRIO, typename QS, int BW = 4, bool FILTER = false>
__device__ __forceinline__ void quad_closest(const TraceParams& p, const QS& st, int c,
                                             const vec3f eye, const vec3f dir, const vec3f inv, float& tbest,
                                             uint32_t& ibest, float& bu, float& bv, unsigned long long& cn,
                                             unsigned long long& ct, uint32_t fray = 0) {
    // One iteration: the pending leaf (if any), then the pop that follows it, then the node visit —
    // a leaf and the next node share an iteration (one loop overhead and one divergent pass fewer
    // per leaf); the per-ray sequence of leaf tests, pops and node visits is trace_pixel's.
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    if (COUNT && !p.num_tris && c == 0) ++cn;  // an empty scene: the all-empty root record orc_bvh_trace visits
    uint32_t iter = 0;
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, cnt = ((next >> 27) & 15u) + 1u;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                const uint32_t k = first + k0 + c;
                float t = __builtin_inff(), u = 0.f, v = 0.f;
                uint32_t id = NO_TRI;
                if (k0 + c < cnt) {
                    // per-lane record loads (the group staged through an LDS tile as contiguous 16-B
                    // pieces was measured against this and not kept: DESIGN.md §5)
                    const float4 a = p.tris[3 * k + 0], b = p.tris[3 * k + 1], cc = p.tris[3 * k + 2];
                    float tt, uu, vv;
                    bool acc = tri_test(a, b, cc, eye, dir, tt, uu, vv) && tt > 0.0f && tt < 3.40282347e+38f;
                    if constexpr (FILTER) acc = acc && tt <= tbest && filter_accept<true>(p, fray, k, f2u(a.w), dir, tt);
                    if (acc) {
                        t = tt;
                        id = f2u(a.w);
                        u = uu;
                        v = vv;
                    }
                }
                quad_min_hit(t, id, u, v);
                if (t < tbest || (t == tbest && id < ibest)) {
                    tbest = t;
                    ibest = id;
                    bu = u;
                    bv = v;
                }
            }
            if (COUNT && c == 0) ct += cnt;
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            bool found = false;
            while (sp > 0) {
                --sp;
                uint32_t ref;
                float tt;
                st.get(sp, ref, tt);
                if (!(tt > tbest)) {
                    next = ref;
                    found = true;
                    break;
                }
            }
            if (!found) break;
            if (next & LEAF_BIT) continue;  // a popped leaf: tested at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = quad_visit_w<BW>(p, next, c, eye, inv, tbest, true, st, sp);
        // more node visits in the same iteration while the nearest child is internal (same
        // sequence; a second visit halved the loop overhead on descents: armadillo proxy -3 %, merged
        // proxy -9 %)
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = quad_visit_w<BW>(p, next, c, eye, inv, tbest, true, st, sp);
        }
    }
}

// Any-hit segment o + s*d, 0 < s < 1 (shadow_ray's loop). Within a leaf the triangles are tested
// four at a time; the counter takes the tests up to the first occluder in leaf order, as the
// sequential loop of orc_bvh_shadow stops there.
// FILTER, fray: as in quad_closest; an occluder is a triangle the filter accepts.
template <bool COUNT, uint32_t PRIO, typename QS, int BW = 4, bool FILTER = false>
__device__ __forceinline__ bool quad_anyhit(const TraceParams& p, const QS& st, int c,
                                            const vec3f o, const vec3f d, unsigned long long& cn,
                                            unsigned long long& ct, uint32_t fray = 0) {
    const vec3f inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
    int sp = 0;
    uint32_t next = 0, iter = 0;
    for (;;) {  // leaf, pop, node visit in one iteration, as in quad_closest
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, cnt = ((next >> 27) & 15u) + 1u;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                const uint32_t k = first + k0 + c;
                uint32_t occ_at = 4;  // slot of the first occluder in this group of four
                if (k0 + c < cnt) {
                    float t, u, v;
                    if (tri_test(p.tris[3 * k + 0], p.tris[3 * k + 1], p.tris[3 * k + 2], o, d, t, u, v) &&
                        t > 0.0f && t < 1.0f) {
                        if constexpr (FILTER) {
                            if (filter_accept<false>(p, fray, k, 0u, d, t)) occ_at = (uint32_t)c;
                        } else {
                            occ_at = (uint32_t)c;
                        }
                    }
                }
                occ_at = min(occ_at, dpp_u<QP_X1>(occ_at));
                occ_at = min(occ_at, dpp_u<QP_X2>(occ_at));
                if (occ_at < 4) {
                    if (COUNT && c == 0) ct += occ_at + 1;
                    return true;
                }
                if (COUNT && c == 0) ct += min(4u, cnt - k0);
            }
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            if (sp == 0) return false;
            --sp;
            float tt;
            st.get(sp, next, tt);
            if (next & LEAF_BIT) continue;  // a popped leaf: tested at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = quad_visit_w<BW>(p, next, c, o, inv, 1.0f, false, st, sp);
        if (next != EMPTY_REF && !(next & LEAF_BIT)) {  // second node visit, as in quad_closest
            if (COUNT && c == 0) ++cn;
            next = quad_visit_w<BW>(p, next, c, o, inv, 1.0f, false, st, sp);
        }
    }
}

// The stack of ray `ray` of this workgroup over the LDS array s: its overflow slot is the ray's
// index in the persistent grid.
template <int LDS_N, int RAYS>
__device__ __forceinline__ QStack<LDS_N, RAYS> quad_stack(const TraceParams& p, uint2 (*s)[RAYS], int ray) {
    QStack<LDS_N, RAYS> st;
    st.s = s;
    st.ray = ray;
    st.g_ref = p.ovf_ref;
    st.g_t = p.ovf_t;
    st.slot = blockIdx.x * RAYS + ray;
    st.stride = p.ovf_stride;
    return st;
}

template <bool COUNT, int LDS_N, uint32_t PRIO, int SH, bool DIAG = false, int BW = 4>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : SH == SH_FUSED ? QUAD_WAVES_FUSED
                                                                                               : QUAD_WAVES))) void
k_trace_quad(const TraceParams p) {
    static_assert(SH == SH_NONE || SH == SH_FUSED, "quad kernel: primary or fused shadow rays");
    static_assert(!DIAG || COUNT, "the diagnostic build counts work");
    const uint64_t t_start = DIAG ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t diag_work = 0;
    __shared__ uint2 s_stk[LDS_N][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<LDS_N> st = quad_stack<LDS_N>(p, s_stk, w * 16 + q);
    const uint32_t tiles_x = (p.width + QTW - 1) / QTW, tiles_y = (p.local_rows + QTH - 1) / QTH;
    const uint32_t ntiles = tiles_x * tiles_y;
    const uint32_t nwaves = gridDim.x * WAVES;
    const vec3f eye = v3(p.eye[0], p.eye[1], p.eye[2]);
    unsigned long long cn = 0, ct = 0, ch = 0, csh[3] = {0, 0, 0};
    // Tile order. Static: wave g of the grid takes tiles g, g + G, ... (G = waves in the grid).
    // Block-dynamic (p.sched == 1): the block's share of the frame — tiles b, b + B, b + 2B, ...
    // (B = blocks), in screen order — is handed to its four waves one tile at a time from an LDS
    // ticket, so a wave that drew a heavy (silhouette) tile does not also own its fixed share of
    // the rest: list scheduling inside the CU, no global atomics.
    // XCD-aware: with a grid that is a multiple of 8 blocks (blocks are placed on the 8 XCDs round
    // robin, block b on XCD b % 8) runs of 8 horizontally adjacent tiles (32 pixels = one 128-B line
    // per row of each 4-B plane) belong to one XCD, so partial lines merge in that XCD's L2 before
    // they are written back; the XCD's runs are dealt to its blocks tile by tile.
    // Cost-ordered (p.sched == 2, p.tile_cost): the block's share is handed out longest first, by
    // the time each tile took in the previous trace of this render target (LPT list scheduling;
    // tile_cost holds it, in 10-ns s_memrealtime ticks, rewritten as the tiles complete). The heavy
    // silhouette tiles then start first instead of whenever screen order reaches them. First trace
    // (all costs zero): screen order. Frames do not depend on the order.
    __shared__ uint32_t s_ticket;
    __shared__ uint32_t s_order[LPT_MAX];
    const bool dyn = p.sched >= 1;
    const bool xcd_map = dyn && (gridDim.x & 7u) == 0;
    const uint32_t xcd = blockIdx.x & 7u, xj = blockIdx.x >> 3, xblocks = gridDim.x >> 3;
    auto tile_of = [&](uint32_t k) -> uint32_t {
        if (!xcd_map) return blockIdx.x + k * gridDim.x;
        // this XCD's local tile, dealt tile by tile over its blocks (whole runs to one block's four
        // waves were measured and not kept: DESIGN.md §5)
        const uint32_t l = xj + k * xblocks;
        return 8u * (xcd + 8u * (l >> 3)) + (l & 7u);
    };
    const bool lpt = p.sched == 2 && p.tile_cost != nullptr && lpt_share_fits(ntiles, gridDim.x);
    if (lpt) {  // sort the share by descending cost (bitonic, in LDS; key = cost << 9 | (511 - k))
        // Keyed by run cost: a run (8 horizontally adjacent tiles, one 128-B line per row of each 4-B
        // plane) is dealt to 8 workgroups of one XCD, tile j to the j-th; when each of them orders its
        // share by its own tiles' costs, a run's tiles complete at different times and the L2 writes
        // its lines back in pieces (WRITE_SIZE 1.56x the planes' bytes on C2). Keyed by the run's
        // summed cost, the 8 workgroups order their shares alike and a run's tiles complete together.
        // Run-cost keys need the 8 workgroups of a run to share their share indices (xblocks % 8 == 0).
        const bool run_cost = (xblocks & 7u) == 0;
        for (uint32_t k = tid; k < LPT_MAX; k += BLOCK) {
            const uint32_t tk = tile_of(k);
            uint32_t cst = 0u;
            if (tk < ntiles) {
                if (run_cost) {  // the run's tiles: tk & ~7 .. (tk | 7), those inside the frame
                    for (uint32_t j = tk & ~7u; j <= (tk | 7u) && j < ntiles; ++j) cst += min(p.tile_cost[j], (1u << 18) - 1u);
                    cst = min(cst, (1u << 22) - 2u) + 1u;
                } else {
                    cst = min(p.tile_cost[tk], (1u << 22) - 1u) + 1u;
                }
            }
            s_order[k] = (cst << 9) | (LPT_MAX - 1u - k);
        }
        __syncthreads();
        for (uint32_t size = 2; size <= LPT_MAX; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t k = tid; k < LPT_MAX; k += BLOCK) {
                    const uint32_t o = k ^ stride;
                    if (o > k) {
                        const uint32_t a = s_order[k], b = s_order[o];
                        const bool desc = (k & size) == 0;  // descending runs first: final order descending
                        if (desc ? a < b : a > b) {
                            s_order[k] = b;
                            s_order[o] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (uint32_t k = tid; k < LPT_MAX; k += BLOCK) s_order[k] = LPT_MAX - 1u - (s_order[k] & (LPT_MAX - 1u));
    }
    auto pick = [&](uint32_t r) -> uint32_t { return tile_of(lpt ? (r < LPT_MAX ? s_order[r] : LPT_MAX) : r); };
    if (tid == 0) s_ticket = WAVES;
    __syncthreads();
    for (uint32_t i = dyn ? pick((uint32_t)w) : blockIdx.x * WAVES + w; i < ntiles;) {
        uint32_t knext = 0;
        if (dyn) {
            if (lane == 0) knext = atomicAdd(&s_ticket, 1u);
            knext = __builtin_amdgcn_readfirstlane(knext);
        }
        const uint32_t tile = i;
        const uint32_t x = (i % tiles_x) * QTW + (q % QTW);
        const uint32_t lr = (i / tiles_x) * QTH + (q / QTW);
        const uint32_t gy = lr < p.local_rows ? global_row(p, lr) : p.height;
        i = dyn ? pick(knext) : i + nwaves;
        if (x >= p.width || gy >= p.height) continue;  // whole quads only
        const uint64_t tile_t0 = lpt ? __builtin_amdgcn_s_memrealtime() : 0;
        __builtin_amdgcn_s_setprio(0);
        const vec3f dir = primary_dir(p, x, gy);
        float tbest = __builtin_inff(), bu = 0.f, bv = 0.f;
        uint32_t ibest = NO_TRI;
        const vec3f inv = v3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
        const unsigned long long before_work = cn + ct;
        quad_closest<COUNT, PRIO, QStack<LDS_N>, BW>(p, st, c, eye, dir, inv, tbest, ibest, bu, bv, cn, ct);
        if (DIAG) diag_add_tile(diag_work, cn + ct - before_work);  // the tile's longest ray, summed per wave
        // 32-bit pixel offset (planes hold < 2^32 pixels): one VGPR live across the fused shadow ray
        const uint32_t o32 = lr * p.width + x;
        uint32_t packed = MISS_PACKED;
        float nzv = 0.0f;
        if (ibest != NO_TRI) {
            packed = shade_hit(p, ibest, bu, bv, nzv);
            if (COUNT && c == 0) ++ch;
        }
        // one plane per lane of the quad
        if (c == 0) p.packed[(size_t)lr * p.pitch_u32 + x] = packed;
        else if (c == 1) p.tri_id[o32] = ibest;
        else if (c == 2) p.t[o32] = tbest;
        else if (p.nz) p.nz[o32] = nzv;
        if (SH == SH_FUSED) {
            bool occ = false;
            if (ibest != NO_TRI) {
                vec3f so, sd;
                shadow_segment(p, eye, dir, tbest, so, sd);
                occ = quad_anyhit<COUNT, PRIO, QStack<LDS_N>, BW>(p, st, c, so, sd, csh[0], csh[1]);
                if (COUNT && c == 0) csh[2] += occ;
            }
            // one byte per quad (measured, round 4: the tile row's four flags as one aligned 4-B store
            // cost three VGPR spills at 7 waves per SIMD, and the scratch traffic outweighed the stores
            // it saved — WRITE_SIZE 61.4 -> 73.2 MB per C5 frame, the same with no shadow store at all)
            if (c == 0) p.shadow[o32] = occ ? 1 : 0;
        }
        if (lpt && lane == 0) p.tile_cost[tile] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tile_t0);
    }
    flush_counters<COUNT>(p, cn, ct, ch, csh);
    if (DIAG) diag_wave_record(p, w, lane, t_start, diag_work);
}

// Compacted ray quads (TRACE_COMPACT, two launches). k_cull runs one lane per pixel over 8x8 tiles:
// the ray setup and a conservative slab test against the root record's four child boxes (inflated,
// see k_cull). A ray that misses all of them is finished exactly as the quad traversal would finish
// it (no child pushed, empty stack): its own lane writes its miss entries. The others are appended
// to their region of the ray queue (a region = a run of consecutive tiles owned by one workgroup;
// wave ballot + popcount rank and one LDS atomic per wave, no global atomics), and the region's
// count is published. k_trace_rays is persistent: each workgroup scans the region counts in LDS,
// and wave w traces the survivors 16 at a time as ray quads (quad_closest, from the root), batches
// w, w + G, w + 2G, ... of the concatenated queue, so quads are only spent on rays that enter the
// scene and the hard rays are spread over every wave. Frames and COUNT counters are those of
// k_trace_quad / orc_bvh_trace (a culled ray counts the one root record the quad traversal visits).
// Measured: on par with k_trace_quad — the survivors' traversal steps, not the
// culled rays, set the frame time.
constexpr int CULL_TILE = 8;
// LDS prefix table of k_trace_rays (4 B each). 1024 vs 2048: shorter prefix scan, C2/C3 in flight
// +1-2 %
constexpr uint32_t CULL_MAX_REGIONS = 1024;
// waves per SIMD k_cull_deep's registers must allow, k_cull's own 7 (without the bound: 73 VGPRs, 6 waves)
constexpr int CULL_WAVES = 7;

// Second cull level (p.cull_depth 2, non-counting builds). A survivor of the conservative root test
// is decided exactly: the ray k_trace_rays would rebuild (primary_dir, IEEE 1/dir) against the root
// record's own child boxes with child_hit and tbest = +inf — quad_visit's operations on its operands,
// so an empty all-NaN child fails and inv = +-inf behaves as it does there. With no hit found the
// traversal visits every root child the ray enters (nothing lowers tbest, so no pop is skipped): if
// all of them are internal and the ray hits none of their child boxes it ends as a miss there, and
// k_cull writes that miss. An entered leaf keeps the ray. The records are wave-uniform: a child
// record is read by scalar loads (constant address space, as k_trace_packet reads its node), and only
// when some lane of the wave enters it; it is read from p.nodes on every launch (a refit rewrites it).
// Measured on C3: 22 % fewer batches, k_trace_rays 3 % shorter, k_cull 21 us longer (the
// dependent scalar loads and IEEE divides of the waves along the silhouette): slower, so depth 1 is the
// default and this kernel is kept for A/B runs (BM_PARAM_CULL_DEPTH 2).
typedef uint32_t cull_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(4))) const cull_u32x2 cull_cuint2;
typedef __attribute__((address_space(4))) const uint32_t cull_cuint;

// Does the ray hit any child box of record `node` (wave-uniform)? Exact, tbest = +inf.
__device__ __forceinline__ bool record_hit(const uint4* nodes, uint32_t node, const vec3f o, const vec3f inv) {
    // two child boxes per pass of a rolled loop (12 SGPRs: the whole record at once spilled SGPRs)
    cull_cuint2* nd = (cull_cuint2*)(nodes) + 16 * (size_t)node;  // generic -> constant address space (a C cast)
    bool any = false;
#pragma unroll 1
    for (uint32_t h = 0; h < 2; ++h) {
        const cull_u32x2 lx = nd[h], ly = nd[2 + h], lz = nd[4 + h], hx = nd[6 + h], hy = nd[8 + h], hz = nd[10 + h];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float lo[3] = {u2f(lx[j]), u2f(ly[j]), u2f(lz[j])}, hi[3] = {u2f(hx[j]), u2f(hy[j]), u2f(hz[j])};
            float tn;
            any |= child_hit(lo, hi, o, inv, __builtin_inff(), tn);
        }
    }
    return any;
}

// The cull of both kernels below. DEEP: with the second level (compiled apart, so that the one-level
// kernel stays the code it was).
template <bool COUNT, int SH, bool DEEP>
__device__ __forceinline__ void cull_tiles(const TraceParams& p) {
    static_assert(!(COUNT && DEEP), "counting builds keep the one-level cull (the oracle's counters)");
    __shared__ uint32_t s_n;
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const uint32_t tiles_x = (p.width + CULL_TILE - 1) / CULL_TILE;
    const uint32_t ntiles = tiles_x * ((p.local_rows + CULL_TILE - 1) / CULL_TILE);
    const uint32_t t0 = blockIdx.x * p.rayq_tpr, t1 = min(t0 + p.rayq_tpr, ntiles);
    uint32_t* region = p.rayq + (size_t)blockIdx.x * p.rayq_region;
    const vec3f eye = v3(p.eye[0], p.eye[1], p.eye[2]);
    // Conservative root cull: the root's four child boxes, each inflated by m = 2^-12 x the
    // scene-and-eye scale, against the exact ray direction with the hardware reciprocal (1 ulp)
    // for 1/d. Its slab distances deviate from the exact test's by ~1e-7 of |box - eye| <= 2 x
    // scale, far inside m, so a culled ray misses every child under the exact test (BuildTree.cu
    // semantics as in quad_visit); rays near the margin just take the exact traversal. Empty
    // children are all-NaN and never pass. Near-axis directions (|d| < 2^-100: reciprocal
    // overflow, 0 x inf) are never culled.
    const uint4* rn = p.nodes;
    const uint4 rlx = rn[0], rly = rn[1], rlz = rn[2], rhx = rn[3], rhy = rn[4], rhz = rn[5];
    const uint32_t LX[4] = {rlx.x, rlx.y, rlx.z, rlx.w}, LY[4] = {rly.x, rly.y, rly.z, rly.w};
    const uint32_t LZ[4] = {rlz.x, rlz.y, rlz.z, rlz.w}, HX[4] = {rhx.x, rhx.y, rhx.z, rhx.w};
    const uint32_t HY[4] = {rhy.x, rhy.y, rhy.z, rhy.w}, HZ[4] = {rhz.x, rhz.y, rhz.z, rhz.w};
    float scale = fmaxf(fabsf(eye.x), fmaxf(fabsf(eye.y), fabsf(eye.z)));
#pragma unroll
    for (int k = 0; k < 4; ++k)
        scale = fmaxf(scale, fmaxf(fmaxf(fmaxf(fabsf(u2f(LX[k])), fabsf(u2f(LY[k]))), fabsf(u2f(LZ[k]))),
                                   fmaxf(fmaxf(fabsf(u2f(HX[k])), fabsf(u2f(HY[k]))), fabsf(u2f(HZ[k])))));
    const float margin = scale * 0x1p-12f;
    float cb[4][6], ub[6] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""),
                             __builtin_nanf(""), __builtin_nanf("")};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cb[k][0] = u2f(LX[k]) - margin, cb[k][1] = u2f(LY[k]) - margin, cb[k][2] = u2f(LZ[k]) - margin;
        cb[k][3] = u2f(HX[k]) + margin, cb[k][4] = u2f(HY[k]) + margin, cb[k][5] = u2f(HZ[k]) + margin;
#pragma unroll
        for (int a = 0; a < 3; ++a) ub[a] = fminf(ub[a], cb[k][a]), ub[3 + a] = fmaxf(ub[3 + a], cb[k][3 + a]);
    }
    const bool any_tris = p.num_tris != 0;
    unsigned long long cn = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    // Four tiles per step with their camera-table loads issued together (the only dependent loads
    // of a ray's setup), so a wave waits for one load latency per four tiles.
    constexpr int UNR = 4;
    for (uint32_t i0 = t0 + w; i0 < t1; i0 += UNR * WAVES) {
        float crx[UNR], cry[UNR];
        uint32_t cx[UNR], clr[UNR];
        bool cval[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const uint32_t i = i0 + u * WAVES;
            cx[u] = (i % tiles_x) * CULL_TILE + (lane & 7);
            clr[u] = (i / tiles_x) * CULL_TILE + (lane >> 3);
            const uint32_t gy = clr[u] < p.local_rows ? global_row(p, clr[u]) : p.height;
            cval[u] = i < t1 && cx[u] < p.width && gy < p.height;
            crx[u] = cval[u] ? p.rx[cx[u]] : 0.f;
            cry[u] = cval[u] ? p.ry[gy] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (i0 + u * WAVES >= t1) break;
            const uint32_t x = cx[u], lr = clr[u];
            bool enter = false;
            if (cval[u]) {
                if (any_tris) {
                    const float rx = crx[u], ry = cry[u];
                    // primary_dir from the preloaded tables; with a near-orthonormal orient (host
                    // check, p.fast_cull) the cull may use the 1-ulp reciprocal square root: the
                    // direction then deviates by ~2^-21 relative, inside the margin m
                    const float q2 = p.z2 + rx * rx + ry * ry;
                    const float d = p.fast_cull ? __builtin_amdgcn_rsqf(q2) : 1.f / sqrtf(q2);
                    const vec3f r = v3(rx * d, ry * d, p.zoom * d);
                    const float* om = p.orient;
                    const vec3f dir = v3((om[0] * r.x + om[3] * r.y) + om[6] * r.z, (om[1] * r.x + om[4] * r.y) + om[7] * r.z,
                                         (om[2] * r.x + om[5] * r.y) + om[8] * r.z);
                    const bool tiny = !(fabsf(dir.x) >= 0x1p-100f && fabsf(dir.y) >= 0x1p-100f && fabsf(dir.z) >= 0x1p-100f);
                    const vec3f inv = v3(__builtin_amdgcn_rcpf(dir.x), __builtin_amdgcn_rcpf(dir.y), __builtin_amdgcn_rcpf(dir.z));
                    // union of the inflated children first (monotone slab distances: a child hit is a
                    // union hit), then the children themselves
                    float tn;
                    enter = tiny;
                    if (!tiny && child_hit(&ub[0], &ub[3], eye, inv, __builtin_inff(), tn)) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) enter |= child_hit(&cb[k][0], &cb[k][3], eye, inv, __builtin_inff(), tn);
                    }
                }
                if (COUNT && !enter) ++cn;  // the root record the quad traversal would visit (an empty scene's too)
                // second level, decided for the wave's survivors only: tiles away from the model
                // skip it on one scalar test
                if (DEEP && ballot(enter)) {
                    // the ray as k_trace_rays rebuilds it: primary_dir's operations on the table
                    // values loaded above (rx = p.rx[x], ry = p.ry[global_row(p, lr)]), IEEE 1/dir
                    const float rx = crx[u], ry = cry[u];
                    const float d = 1.f / sqrtf(p.z2 + rx * rx + ry * ry);
                    const vec3f dir = orient_mul(p.orient, v3(rx * d, ry * d, p.zoom * d));
                    const vec3f inv = v3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
                    // One root child per pass of a rolled loop, its box and ref re-read from the root
                    // record by scalar loads: unrolled over the children (and the four tiles of a
                    // step) the 16 grandchild boxes cost 27 VGPRs and spilled SGPRs
                    cull_cuint* rw = (cull_cuint*)(p.nodes);
                    bool keep = false;
#pragma unroll 1
                    for (uint32_t k = 0; k < 4; ++k) {
                        const float lo[3] = {u2f(rw[k]), u2f(rw[4 + k]), u2f(rw[8 + k])};
                        const float hi[3] = {u2f(rw[12 + k]), u2f(rw[16 + k]), u2f(rw[20 + k])};
                        const uint32_t ref = rw[24 + k];
                        float tn;
                        const bool in_k = enter && child_hit(lo, hi, eye, inv, __builtin_inff(), tn);
                        if (ref & LEAF_BIT) {  // a leaf (or an empty slot, which no ray enters)
                            keep |= in_k;
                        } else if (ballot(in_k)) {
                            keep |= in_k && record_hit(p.nodes, ref, eye, inv);
                        }
                    }
                    enter = keep;
                }
                if (!enter) {
                    const size_t o = (size_t)lr * p.width + x;
                    p.packed[(size_t)lr * p.pitch_u32 + x] = MISS_PACKED;
                    p.tri_id[o] = NO_TRI;
                    p.t[o] = __builtin_inff();
                    if (p.nz) p.nz[o] = 0.0f;
                    if (SH == SH_FUSED) p.shadow[o] = 0;
                }
            }
            const unsigned long long mask = ballot(enter);
            if (mask) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_n, (uint32_t)__popcll(mask));
                base = __builtin_amdgcn_readfirstlane(base);
                if (enter) region[base + (uint32_t)__popcll(mask & below)] = x | (lr << 16);
            }
        }
    }
    __syncthreads();
    if (tid == 0) p.rayq_count[blockIdx.x] = s_n;
    if (COUNT) atomicAdd(&p.counters[0], cn);
}

template <bool COUNT, int SH>
__global__ __launch_bounds__(BLOCK) void k_cull(const TraceParams p) {
    cull_tiles<COUNT, SH, false>(p);
}

// k_cull with the second level (p.cull_depth 2; non-counting traces only).
template <int SH>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(CULL_WAVES))) void k_cull_deep(const TraceParams p) {
    cull_tiles<false, SH, true>(p);
}

template <bool COUNT, int LDS_N, uint32_t PRIO, int SH, bool DIAG = false>
__global__ __launch_bounds__(BLOCK) void k_trace_rays(const TraceParams p) {
    static_assert(SH == SH_NONE || SH == SH_FUSED, "compact kernels: primary or fused shadow rays");
    static_assert(!DIAG || COUNT, "the diagnostic build counts work");
    const uint64_t t_start = DIAG ? __builtin_amdgcn_s_memrealtime() : 0;
    uint64_t diag_work = 0;
    __shared__ uint2 s_stk[LDS_N][QRAYS];
    __shared__ uint32_t s_pre[CULL_MAX_REGIONS];  // inclusive prefix of the region counts
    __shared__ uint32_t s_wsum[WAVES];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    // ---- inclusive scan of the region counts (every workgroup, into LDS) ----
    const uint32_t nreg = p.rayq_regions;
    constexpr uint32_t PER = CULL_MAX_REGIONS / BLOCK;
    uint32_t v[PER], run = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t r = tid * PER + k;
        run += r < nreg ? p.rayq_count[r] : 0u;
        v[k] = run;
    }
    const uint32_t incl = wave_incl_add(run);  // wave-inclusive scan of the per-thread totals
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    uint32_t off = incl - run;
    for (int k = 0; k < w; ++k) off += s_wsum[k];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) s_pre[tid * PER + k] = v[k] + off;
    __syncthreads();
    const uint32_t total = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    const QStack<LDS_N> st = quad_stack<LDS_N>(p, s_stk, w * 16 + q);
    const vec3f eye = v3(p.eye[0], p.eye[1], p.eye[2]);
    unsigned long long cn = 0, ct = 0, ch = 0, csh[3] = {0, 0, 0};
    const uint32_t nbatch = (total + 15) / 16, nwaves = gridDim.x * WAVES;
    const uint32_t last = nreg ? nreg - 1 : 0;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        const unsigned long long before_work = cn + ct;
        // region of the batch's first survivor (the first r with s_pre[r] > 16 b) by a 64-ary search —
        // each lane reads one segment end, a ballot picks the segment, then its 16 entries the same
        // way: two LDS reads where a binary search over 1,024 regions took ten dependent ones; each ray
        // then steps forward over the (rare) region ends inside its batch
        static_assert(CULL_MAX_REGIONS <= 1024, "64 segments of 16 regions");
        uint32_t lo;
        {
            const uint32_t s0 = b * 16;
            const unsigned long long m1 = ballot(s_pre[min(16u * (uint32_t)lane + 15u, last)] > s0);
            const uint32_t seg = m1 ? (uint32_t)__ffsll((long long)m1) - 1u : 63u;
            const unsigned long long m2 = ballot(s_pre[min(seg * 16u + ((uint32_t)lane & 15u), last)] > s0) & 0xFFFFull;
            lo = min(seg * 16u + (m2 ? (uint32_t)__ffsll((long long)m2) - 1u : 15u), last);
        }
        if (sidx < total) {  // whole quads only
            while (lo < last && s_pre[lo] <= sidx) ++lo;
            const uint32_t before = lo ? s_pre[lo - 1] : 0u;
            const uint32_t pix = p.rayq[(size_t)lo * p.rayq_region + (sidx - before)];
            const uint32_t x = pix & 0xFFFFu, lr = pix >> 16;
            __builtin_amdgcn_s_setprio(0);
            const vec3f dir = primary_dir(p, x, global_row(p, lr));
            const vec3f inv = v3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
            float tbest = __builtin_inff(), bu = 0.f, bv = 0.f;
            uint32_t ibest = NO_TRI;
            quad_closest<COUNT, PRIO>(p, st, c, eye, dir, inv, tbest, ibest, bu, bv, cn, ct);
            const size_t o = (size_t)lr * p.width + x;
            // the finish of k_trace_quad with a 64-bit pixel offset (one shared helper for the two
            // changed the instruction counts of the counting fused-shadow kernels, so each keeps its own)
            uint32_t packed = MISS_PACKED;
            float nzv = 0.0f;
            if (ibest != NO_TRI) {
                packed = shade_hit(p, ibest, bu, bv, nzv);
                if (COUNT && c == 0) ++ch;
            }
            if (c == 0) p.packed[(size_t)lr * p.pitch_u32 + x] = packed;
            else if (c == 1) p.tri_id[o] = ibest;
            else if (c == 2) p.t[o] = tbest;
            else if (p.nz) p.nz[o] = nzv;
            if (SH == SH_FUSED) {
                bool occ = false;
                if (ibest != NO_TRI) {
                    vec3f so, sd;
                    shadow_segment(p, eye, dir, tbest, so, sd);
                    occ = quad_anyhit<COUNT, PRIO>(p, st, c, so, sd, csh[0], csh[1]);
                    if (COUNT && c == 0) csh[2] += occ;
                }
                if (c == 0) p.shadow[o] = occ ? 1 : 0;
            }
        }
        if (DIAG) diag_add_tile(diag_work, cn + ct - before_work);
    }
    flush_counters<COUNT>(p, cn, ct, ch, csh);
    if (DIAG) diag_wave_record(p, w, lane, t_start, diag_work);
}

}  // namespace
}  // namespace bm
