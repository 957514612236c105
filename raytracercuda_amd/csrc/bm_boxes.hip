// bm_boxes.hip — box overlap queries: for each axis-aligned box of a caller's batch in device memory, the
// triangles of the scene that intersect it (bm_scene_overlap_boxes): how many (BM_BOXES_COUNT), whether
// any (BM_BOXES_ANY), or their ids into the box's segment of a CSR list (BM_BOXES_LIST). "Intersects" is
// the reference's own triangle/box separating-axis test, tri_box of bm_sat_dev.h, on the triangle as the
// build's 48-byte record holds it (v0, v0 + e1, v0 + e2).
//   k_overlap_boxes  persistent grid; a wave takes batches of 16 consecutive boxes (512 contiguous
//                    bytes), lane 4q+c works for box 16b+q — the shape of k_closest_points
// The traversal (quad_overlap) has no order and no bound: lane c tests child c's box against the query
// box with the SAT's own AABB arithmetic (fl(lo - c) <= h && fl(hi - c) >= -h per axis), the kept children
// are ranked by slot, the first followed and the others pushed. Float subtraction is monotonic, so a box
// that holds an accepted triangle's vertices passes that test whenever the triangle passed the SAT's AABB
// test: nothing is lost, and the result is bit for bit what tri_box gives over ALL triangles.
// Nothing is decided by an atomic: the order of a LIST segment is the traversal's, the same on every grid.
#include "bm_query_dev.h"
#include "bm_sat_dev.h"

namespace bm {
namespace {

// Node step: lane c loads child c of the 128-B record as nearest_visit does and keeps it when it is not an
// empty slot and its box meets the query box on every axis. The positive form of the comparisons: an empty
// slot's NaN box fails them by itself. The kept children are ranked by slot with quad_visit's DPP exchange
// (key = slot), ranks 1..nh-1 pushed highest slot first, the lowest kept slot returned to all four lanes
// (EMPTY_REF when none is kept).
template <typename QS>
__device__ __forceinline__ uint32_t box_visit(const TraceParams& p, uint32_t node, int c, const float* bc,
                                              const float* hs, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const float lx = u2f(nd[0]), ly = u2f(nd[4]), lz = u2f(nd[8]);
    const float hx = u2f(nd[12]), hy = u2f(nd[16]), hz = u2f(nd[20]);
    const uint32_t ref = nd[24];
    const bool h = (ref != EMPTY_REF) & (lx - bc[0] <= hs[0]) & (hx - bc[0] >= -hs[0]) & (ly - bc[1] <= hs[1]) &
                   (hy - bc[1] >= -hs[1]) & (lz - bc[2] <= hs[2]) & (hz - bc[2] >= -hs[2]);
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

// The triangles of one box over the quad. One iteration is quad_nearest's: the pending leaf, the pop that
// follows it, the node visit(s). At a leaf lane c runs tri_box on triangle k0 + c; the quad sums the accepts.
// MODE BM_BOXES_ANY: returns at the first group with an accept. BM_BOXES_LIST: an accepting lane's slot is
// found + (accepts of the lower lanes of its group), and it stores its id at ids[slot] while slot < cap (ids:
// the start of this box's segment, cap its length). found: |O| on return (ANY: 0 or at least 1), the same
// in every lane of the quad. maxsp (COUNT): the most stack entries held at once.
template <bool COUNT, uint32_t PRIO, uint32_t MODE, typename QS>
__device__ __forceinline__ void quad_overlap(const TraceParams& p, const QS& st, int c, const float* bc, const float* hs,
                                             uint32_t* ids, uint32_t cap, uint32_t& found, unsigned long long& cn,
                                             unsigned long long& ct, int& maxsp) {
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
                    const float tv[9] = {a.x, a.y, a.z, a.x + b.x, a.y + b.y, a.z + b.z, a.x + cc.x, a.y + cc.y, a.z + cc.z};
                    acc = tri_box(bc, hs, tv) ? 1u : 0u;
                    id = f2u(a.w);
                }
                const uint32_t a1 = dpp_u<QP_X1>(acc), a2 = dpp_u<QP_X2>(acc), a3 = dpp_u<QP_X3>(acc);
                if (MODE == BM_BOXES_LIST) {
                    // the accepts of the lanes below c: lane c^1 for odd c, lanes c^2 and c^3 for c >= 2
                    const uint32_t slot = found + ((c & 1) ? a1 : 0u) + ((c & 2) ? a2 + a3 : 0u);
                    if (acc && slot < cap) ids[slot] = id;
                }
                found += (acc + a1) + (a2 + a3);
                if (MODE == BM_BOXES_ANY && found) return;
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
        next = box_visit(p, next, c, bc, hs, st, sp);
        if (COUNT) maxsp = max(maxsp, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = box_visit(p, next, c, bc, hs, st, sp);
            if (COUNT) maxsp = max(maxsp, sp);
        }
    }
}

// waves per SIMD the registers must allow. Below the quad kernels' 7: the straight-line SAT holds the box,
// the three vertices and the three edges at once beside the traversal's state, 111-114 VGPRs. Asked to fit
// 5, 6 or 7 waves the compiler spills 3-9, 22-32 and 30-76 VGPRs to scratch.
constexpr int BOXES_WAVES = 4;

// A box record is two float4: (centre, pad) (half, pad); the four lanes of a quad load the same 32 bytes.
// An invalid box (a non-finite component of the centre or the half-size, or a negative half-size) is
// finished here with count 0, so no NaN reaches the traversal. Launch parameters: q_rays the boxes, q_n
// their number, q_out the count or byte plane (LIST: may be null), q_ent the LIST offsets (n + 1,
// ascending), q_counts the LIST ids.
template <bool COUNT, uint32_t PRIO, uint32_t MODE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : BOXES_WAVES))) void
k_overlap_boxes(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    int maxsp = 0;
    const uint32_t n = p.q_n;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[2 * (size_t)sidx], r1 = p.q_rays[2 * (size_t)sidx + 1];
        const float bc[3] = {r0.x, r0.y, r0.z}, hs[3] = {r1.x, r1.y, r1.z};
        const bool valid = finite3(v3(r0.x, r0.y, r0.z)) && finite3(v3(r1.x, r1.y, r1.z)) && r1.x >= 0.0f &&
                           r1.y >= 0.0f && r1.z >= 0.0f;  // false for NaN
        __builtin_amdgcn_s_setprio(0);
        uint32_t found = 0;
        if (valid) {
            uint32_t* ids = nullptr;
            uint32_t cap = 0;
            if (MODE == BM_BOXES_LIST) {
                const uint32_t o0 = p.q_ent[sidx], o1 = p.q_ent[sidx + 1];
                ids = p.q_counts + o0;
                cap = o1 > o0 ? o1 - o0 : 0u;
            }
            quad_overlap<COUNT, PRIO, MODE>(p, st, c, bc, hs, ids, cap, found, cn, ct, maxsp);
            if (COUNT && c == 0) ch += MODE == BM_BOXES_ANY ? (found ? 1u : 0u) : found;
        }
        if (c == 0) {
            if (MODE == BM_BOXES_ANY) reinterpret_cast<uint8_t*>(p.q_out)[sidx] = found ? 1 : 0;
            else if (MODE == BM_BOXES_COUNT || p.q_out) reinterpret_cast<uint32_t*>(p.q_out)[sidx] = found;
        }
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

template <uint32_t MODE>
void launch_mode(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_overlap_boxes<true, 1, MODE>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_overlap_boxes<false, 0, MODE>, p, s, nullptr);
    else launch_persistent(k_overlap_boxes<false, 1, MODE>, p, s, nullptr);
}

}  // namespace

hipError_t launch_overlap_boxes(const TraceParams& p, uint32_t mode, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_BOXES_LIST || (mode != BM_BOXES_LIST && !p.q_out) ||
        (mode == BM_BOXES_LIST && (!p.q_ent || !p.q_counts)))
        return hipErrorInvalidValue;
    if (mode == BM_BOXES_COUNT) launch_mode<BM_BOXES_COUNT>(p, count, s);
    else if (mode == BM_BOXES_ANY) launch_mode<BM_BOXES_ANY>(p, count, s);
    else launch_mode<BM_BOXES_LIST>(p, count, s);
    return hipGetLastError();
}

}  // namespace bm
