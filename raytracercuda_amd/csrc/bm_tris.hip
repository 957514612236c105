// bm_tris.hip — triangle overlap queries: for each triangle of a caller's batch in device memory, the
// triangles of the scene that intersect it (bm_scene_overlap_triangles): how many (BM_TRIS_COUNT), whether
// any (BM_TRIS_ANY), or their ids into the query's segment of a CSR list (BM_TRIS_LIST). "Intersects" is
// tri_tri of bm_tritri_dev.h, touching included, on the scene triangle as the build's 48-byte record holds
// it (v0, v0 + e1, v0 + e2).
//   k_overlap_tris  persistent grid; a wave takes batches of 16 consecutive query triangles (768 contiguous
//                   bytes), lane 4q+c works for query 16b+q — the shape of k_overlap_boxes
// The traversal (quad_overlap_tris) has no order and no bound: lane c keeps child c when its box meets the
// query triangle's own bounds, lo <= qhi && hi >= qlo per axis on the raw coordinates, no arithmetic at all.
// tri_tri's AABB part is the same comparison on the scene triangle's own bounds, so a box that holds an
// accepted triangle's vertices passes: nothing is lost, and the result is bit for bit what tri_tri gives over
// ALL triangles. Nothing is decided by an atomic: the order of a LIST segment is the
// traversal's, the same on every grid.
#include "bm_query_dev.h"
#include "bm_tritri_dev.h"

namespace bm {
namespace {

// Node step: box_visit of bm_boxes.hip with the query's bounds in the box's place. Lane c loads child c of
// the 128-B record and keeps it when it is not an empty slot and its box meets [qlo, qhi] on every axis. The
// positive form of the comparisons: an empty slot's NaN box fails them by itself. The kept children are
// ranked by slot, ranks 1..nh-1 pushed highest slot first, the lowest kept slot returned to all four lanes
// (EMPTY_REF when none is kept).
template <typename QS>
__device__ __forceinline__ uint32_t tri_visit(const TraceParams& p, uint32_t node, int c, const float* qlo,
                                              const float* qhi, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const float lx = u2f(nd[0]), ly = u2f(nd[4]), lz = u2f(nd[8]);
    const float hx = u2f(nd[12]), hy = u2f(nd[16]), hz = u2f(nd[20]);
    const uint32_t ref = nd[24];
    const bool h = (ref != EMPTY_REF) & (lx <= qhi[0]) & (hx >= qlo[0]) & (ly <= qhi[1]) & (hy >= qlo[1]) &
                   (lz <= qhi[2]) & (hz >= qlo[2]);
    const uint32_t key = h ? (uint32_t)c : ~0u;
    const uint32_t k1 = dpp_u<QP_X1>(key), k2 = dpp_u<QP_X2>(key), k3 = dpp_u<QP_X3>(key);
    const uint32_t rank = (uint32_t)(k1 < key) + (uint32_t)(k2 < key) + (uint32_t)(k3 < key);
    uint32_t nh = h ? 4u : rank;  // a dropped child's key ~0u ranks after every kept one: its rank is their count
    nh = min(nh, dpp_u<QP_X1>(nh));
    nh = min(nh, dpp_u<QP_X2>(nh));
    if (h && rank > 0) st.put(sp + (int)(nh - 1u - rank), ref, 0.0f);
    sp += max((int)nh - 1, 0);
    uint32_t nx = (h && rank == 0) ? ref : EMPTY_REF;
    nx = min(nx, dpp_u<QP_X1>(nx));
    nx = min(nx, dpp_u<QP_X2>(nx));
    return nx;
}

// The triangles of one query triangle over the quad: quad_overlap of bm_boxes.hip with tri_tri at the leaves.
// skip: a triangle id that is never reported (NO_TRI: none; no scene triangle has that id). The filter runs
// on candidates the test has accepted. found: |O| on return (ANY: 0 or at least 1), the same in every lane
// of the quad. maxsp (COUNT): the most stack entries held at once.
template <bool COUNT, uint32_t PRIO, uint32_t MODE, typename QS>
__device__ __forceinline__ void quad_overlap_tris(const TraceParams& p, const QS& st, int c, const TriQuery& t,
                                                  uint32_t skip, uint32_t* ids, uint32_t cap, uint32_t& found,
                                                  unsigned long long& cn, unsigned long long& ct, int& maxsp) {
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    uint32_t iter = 0;
    for (;;) {
        prio_boost<PRIO>(p, iter);
        if (next != EMPTY_REF && (next & LEAF_BIT)) {
            const uint32_t first = next & FIRST_MASK, cnt = ((next >> 27) & 15u) + 1u;
            if (COUNT && c == 0) ct += cnt;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 4) {
                const uint32_t k = first + k0 + c;
                uint32_t acc = 0, id = NO_TRI;
                if (k0 + c < cnt) {
                    const float4 a = p.tris[3 * k + 0], b = p.tris[3 * k + 1], cc = p.tris[3 * k + 2];
                    const float b0[3] = {a.x, a.y, a.z}, b1[3] = {a.x + b.x, a.y + b.y, a.z + b.z},
                                b2[3] = {a.x + cc.x, a.y + cc.y, a.z + cc.z};
                    id = f2u(a.w);
                    acc = (tri_tri(t, b0, b1, b2) & (id != skip)) ? 1u : 0u;
                }
                const uint32_t a1 = dpp_u<QP_X1>(acc), a2 = dpp_u<QP_X2>(acc), a3 = dpp_u<QP_X3>(acc);
                if (MODE == BM_TRIS_LIST) {
                    // the accepts of the lanes below c: lane c^1 for odd c, lanes c^2 and c^3 for c >= 2
                    const uint32_t slot = found + ((c & 1) ? a1 : 0u) + ((c & 2) ? a2 + a3 : 0u);
                    if (acc && slot < cap) ids[slot] = id;
                }
                found += (acc + a1) + (a2 + a3);
                if (MODE == BM_TRIS_ANY && found) return;
            }
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            if (sp == 0) return;
            --sp;
            float key;
            st.get(sp, next, key);
            if (next & LEAF_BIT) continue;  // a popped leaf: tested at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = tri_visit(p, next, c, t.qlo, t.qhi, st, sp);
        if (COUNT) maxsp = max(maxsp, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = tri_visit(p, next, c, t.qlo, t.qhi, st, sp);
            if (COUNT) maxsp = max(maxsp, sp);
        }
    }
}

// waves per SIMD the registers must allow: the highest value at which no non-counting instantiation has
// scratch or spills, 91-96 VGPRs. Asked to fit 6 or 7 waves the compiler spills 10-15 and 23-25 VGPRs to
// scratch. The file is built without the SLP vectorizer (build.py): with it the seventeen axes' arithmetic
// is packed into v_pk_* pairs, every instantiation wants some 240 VGPRs and spills about 260 at any setting
// (DESIGN.md §26 has the tables). BM_TRIS_WAVES: an A/B build's other value (tools/build_ab.py).
#ifndef BM_TRIS_WAVES
#define BM_TRIS_WAVES 5
#endif
constexpr int TRIS_WAVES = BM_TRIS_WAVES;

// A query record is three float4: (v0, pad0) (v1, pad1) (v2, pad2); the four lanes of a quad load the same 48
// bytes. An invalid triangle (a non-finite vertex component) is finished here with count 0, so no NaN reaches
// the traversal. Launch parameters: q_rays the triangles, q_n their number, q_flags the call's flags, q_out
// the count or byte plane (LIST: may be null), q_ent the LIST offsets (n + 1, ascending), q_counts the LIST
// ids.
template <bool COUNT, uint32_t PRIO, uint32_t MODE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : TRIS_WAVES))) void
k_overlap_tris(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    int maxsp = 0;
    const uint32_t n = p.q_n;
    const bool skipping = (p.q_flags & BM_TRIS_PAD_SKIP_TRI) != 0;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[3 * (size_t)sidx], r1 = p.q_rays[3 * (size_t)sidx + 1],
                     r2 = p.q_rays[3 * (size_t)sidx + 2];
        const float a0[3] = {r0.x, r0.y, r0.z}, a1[3] = {r1.x, r1.y, r1.z}, a2[3] = {r2.x, r2.y, r2.z};
        const bool valid = finite3(v3(r0.x, r0.y, r0.z)) && finite3(v3(r1.x, r1.y, r1.z)) &&
                           finite3(v3(r2.x, r2.y, r2.z));
        __builtin_amdgcn_s_setprio(0);
        uint32_t found = 0;
        if (valid) {
            uint32_t* ids = nullptr;
            uint32_t cap = 0;
            if (MODE == BM_TRIS_LIST) {
                const uint32_t o0 = p.q_ent[sidx], o1 = p.q_ent[sidx + 1];
                ids = p.q_counts + o0;
                cap = o1 > o0 ? o1 - o0 : 0u;
            }
            TriQuery t;
            tri_query(a0, a1, a2, t);
            quad_overlap_tris<COUNT, PRIO, MODE>(p, st, c, t, skipping ? f2u(r0.w) : NO_TRI, ids, cap, found, cn,
                                                 ct, maxsp);
            if (COUNT && c == 0) ch += MODE == BM_TRIS_ANY ? (found ? 1u : 0u) : found;
        }
        if (c == 0) {
            if (MODE == BM_TRIS_ANY) reinterpret_cast<uint8_t*>(p.q_out)[sidx] = found ? 1 : 0;
            else if (MODE == BM_TRIS_COUNT || p.q_out) reinterpret_cast<uint32_t*>(p.q_out)[sidx] = found;
        }
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

template <uint32_t MODE>
void launch_mode(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_overlap_tris<true, 1, MODE>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_overlap_tris<false, 0, MODE>, p, s, nullptr);
    else launch_persistent(k_overlap_tris<false, 1, MODE>, p, s, nullptr);
}

}  // namespace

hipError_t launch_overlap_triangles(const TraceParams& p, uint32_t mode, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_TRIS_LIST || (mode != BM_TRIS_LIST && !p.q_out) ||
        (mode == BM_TRIS_LIST && (!p.q_ent || !p.q_counts)))
        return hipErrorInvalidValue;
    if (mode == BM_TRIS_COUNT) launch_mode<BM_TRIS_COUNT>(p, count, s);
    else if (mode == BM_TRIS_ANY) launch_mode<BM_TRIS_ANY>(p, count, s);
    else launch_mode<BM_TRIS_LIST>(p, count, s);
    return hipGetLastError();
}

}  // namespace bm
