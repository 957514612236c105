// bm_planes.hip — plane section queries: for each plane of a caller's batch in device memory, the triangles
// of the scene it crosses (bm_scene_section_planes): how many (BM_PLANES_COUNT), whether any (BM_PLANES_ANY),
// or their ids and cut segments into the plane's segment of a CSR list (BM_PLANES_LIST). "Crossed" is stated
// on the meshes' own vertices (include/beam_c.h): s(x) = (n.x*d.x + n.y*d.y) + n.z*d.z with d = x - point, a
// vertex is below when s < 0 and above otherwise, and a triangle is crossed when it has a vertex on each side.
//   k_section_planes  persistent grid; a wave takes batches of 16 consecutive planes (512 contiguous
//                     bytes), lane 4q+c works for plane 16b+q — the shape of k_overlap_boxes
// The traversal (quad_section) has no order and no bound: lane c evaluates s on two corners of child c's box,
// the one that is highest along the normal and the one that is lowest, and keeps the child when the lower is
// below and the upper above. Every operation of s is monotone in each coordinate of x, so s of any point of
// the box lies between the two in the same arithmetic: a box that holds a crossed triangle's vertices passes,
// with no margin, and the result is bit for bit the rule over ALL triangles.
// Nothing is decided by an atomic: the order of a LIST segment is the traversal's, the same on every grid.
#include "bm_query_dev.h"

namespace bm {
namespace {

// s(x) of the header: one rounding per operation, in this order.
__device__ __forceinline__ float plane_side(const float* pt, const float* nr, float x, float y, float z) {
    const float dx = x - pt[0], dy = y - pt[1], dz = z - pt[2];
    return (nr[0] * dx + nr[1] * dy) + nr[2] * dz;
}

// Node step: lane c loads child c of the 128-B record as box_visit does and keeps it when it is not an empty
// slot, the corner lowest along the normal is below the plane and the corner highest along it is above. The
// positive form of the comparisons: an empty slot's NaN box fails them by itself. The kept children are ranked
// by slot with quad_visit's DPP exchange (key = slot), ranks 1..nh-1 pushed highest slot first, the lowest
// kept slot returned to all four lanes (EMPTY_REF when none is kept).
template <typename QS>
__device__ __forceinline__ uint32_t plane_visit(const TraceParams& p, uint32_t node, int c, const float* pt,
                                                const float* nr, const QS& st, int& sp) {
    const uint32_t* nd = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(p.nodes) +
                                                           ((node << 7) | ((uint32_t)c << 2)));
    const float lx = u2f(nd[0]), ly = u2f(nd[4]), lz = u2f(nd[8]);
    const float hx = u2f(nd[12]), hy = u2f(nd[16]), hz = u2f(nd[20]);
    const uint32_t ref = nd[24];
    const bool px = nr[0] >= 0.0f, py = nr[1] >= 0.0f, pz = nr[2] >= 0.0f;
    const float s_upper = plane_side(pt, nr, px ? hx : lx, py ? hy : ly, pz ? hz : lz);
    const float s_lower = plane_side(pt, nr, px ? lx : hx, py ? ly : hy, pz ? lz : hz);
    const bool h = (ref != EMPTY_REF) & (s_lower < 0.0f) & (s_upper >= 0.0f);
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

// The cut of an edge with below end N (s = sn < 0) and above end P (s = sp >= 0): t = sn / (sn - sp), and per
// component t*P + (N - t*N). It depends on the two positions and the plane alone, not on the edge's direction.
__device__ __forceinline__ void edge_cut(const float* N, float sn, const float* P, float sp, float* X) {
    const float t = sn / (sn - sp);
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = t * P[k] + (N[k] - t * N[k]);
}

// The crossed triangles of one plane over the quad. One iteration is quad_overlap's: the pending leaf, the pop
// that follows it, the node visit(s). At a leaf lane c takes triangle k0 + c: its id from the record, its mesh
// by the attribute kernel's search, its index triple and the three positions, three s values; the quad sums
// the accepts. MODE BM_PLANES_ANY: returns at the first group with an accept. BM_PLANES_LIST: an accepting
// lane's slot is found + (accepts of the lower lanes of its group), and while slot < cap it stores its id at
// ids[slot] (ids: the start of this plane's segment, or null) and its segment at segs[2 * slot] (likewise).
// found: |C| on return (ANY: 0 or at least 1), the same in every lane of the quad.
template <bool COUNT, uint32_t PRIO, uint32_t MODE, typename QS>
__device__ __forceinline__ void quad_section(const TraceParams& p, const PlaneParams& x, const QS& st, int c,
                                             const float* pt, const float* nr, uint32_t plane, uint32_t* ids,
                                             float4* segs, uint32_t cap, uint32_t& found, unsigned long long& cn,
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
                float v[3][3] = {}, s[3] = {};
                if (k0 + c < cnt) {
                    id = reinterpret_cast<const uint32_t*>(p.tris)[12 * (size_t)k + 3];  // v0.w of the record
                    if (id < p.num_tris) {
                        uint32_t m = 0;
                        if (x.num_meshes > 1) {  // the last mesh whose offset is <= id, as k_hit_attrs finds it
                            uint32_t hi = x.num_meshes;
                            while (hi - m > 1) {
                                const uint32_t mid = m + ((hi - m) >> 1);
                                if (x.offsets[mid] <= id) m = mid;
                                else hi = mid;
                            }
                        }
                        const AttrMesh* __restrict__ md = x.meshes + m;
                        const uint32_t* __restrict__ ix = md->idx + 3 * (size_t)(id - md->tri_offset);
                        const float* __restrict__ pos = md->slot[BM_VERTEX_DATA_POSITION];
                        bool below[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const float* q = pos + 3 * (size_t)ix[j];
                            v[j][0] = q[0], v[j][1] = q[1], v[j][2] = q[2];
                            s[j] = plane_side(pt, nr, v[j][0], v[j][1], v[j][2]);
                            below[j] = s[j] < 0.0f;
                        }
                        acc = ((below[0] | below[1] | below[2]) & !(below[0] & below[1] & below[2])) ? 1u : 0u;
                    }
                }
                const uint32_t a1 = dpp_u<QP_X1>(acc), a2 = dpp_u<QP_X2>(acc), a3 = dpp_u<QP_X3>(acc);
                if (MODE == BM_PLANES_LIST) {
                    // the accepts of the lanes below c: lane c^1 for odd c, lanes c^2 and c^3 for c >= 2
                    const uint32_t slot = found + ((c & 1) ? a1 : 0u) + ((c & 2) ? a2 + a3 : 0u);
                    if (acc && slot < cap) {
                        if (ids) ids[slot] = id;
                        if (segs) {
                            // going 0 -> 1 -> 2 -> 0 one edge runs from above to below (its cut is a) and one
                            // from below to above (its cut is b)
                            const bool b0 = s[0] < 0.0f, b1 = s[1] < 0.0f, b2 = s[2] < 0.0f;
                            const int dn = (!b0 && b1) ? 0 : (!b1 && b2) ? 1 : 2;  // the down edge starts at dn
                            const int up = (b0 && !b1) ? 0 : (b1 && !b2) ? 1 : 2;  // the up edge starts at up
                            float A[3], B[3], P[3], N[3], sP, sN;
                            // down edge: above end dn, below end dn + 1
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                P[j] = dn == 0 ? v[0][j] : dn == 1 ? v[1][j] : v[2][j];
                                N[j] = dn == 0 ? v[1][j] : dn == 1 ? v[2][j] : v[0][j];
                            }
                            sP = dn == 0 ? s[0] : dn == 1 ? s[1] : s[2];
                            sN = dn == 0 ? s[1] : dn == 1 ? s[2] : s[0];
                            edge_cut(N, sN, P, sP, A);
                            // up edge: below end up, above end up + 1
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                N[j] = up == 0 ? v[0][j] : up == 1 ? v[1][j] : v[2][j];
                                P[j] = up == 0 ? v[1][j] : up == 1 ? v[2][j] : v[0][j];
                            }
                            sN = up == 0 ? s[0] : up == 1 ? s[1] : s[2];
                            sP = up == 0 ? s[1] : up == 1 ? s[2] : s[0];
                            edge_cut(N, sN, P, sP, B);
                            segs[2 * (size_t)slot + 0] = make_float4(A[0], A[1], A[2], u2f(id));
                            segs[2 * (size_t)slot + 1] = make_float4(B[0], B[1], B[2], u2f(plane));
                        }
                    }
                }
                found += (acc + a1) + (a2 + a3);
                if (MODE == BM_PLANES_ANY && found) return;
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
        next = plane_visit(p, next, c, pt, nr, st, sp);
        if (COUNT) maxsp = max(maxsp, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = plane_visit(p, next, c, pt, nr, st, sp);
            if (COUNT) maxsp = max(maxsp, sp);
        }
    }
}

// waves per SIMD the registers must allow: the highest value without scratch or spills. The
// counting and any modes fit 8 (51-53 VGPRs); the list mode holds the three positions and their s values for
// the cuts and, asked to fit 8 (64 VGPRs), spills 10 to scratch: 7.
constexpr int PLANES_WAVES = 8, PLANES_WAVES_LIST = 7;

// A plane record is two float4: (point, pad) (normal, pad); the four lanes of a quad load the same 32 bytes.
// An invalid plane (a non-finite component of the point or the normal, or a normal of all zeros) is finished
// here with count 0, so no NaN reaches the traversal. Launch parameters: q_rays the planes, q_n their number,
// q_out the count or byte plane (LIST: may be null), q_ent the LIST offsets (n + 1, ascending), q_counts the
// LIST ids and x.segs the LIST segments (either may be null).
template <bool COUNT, uint32_t PRIO, uint32_t MODE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : MODE == BM_PLANES_LIST ? PLANES_WAVES_LIST : PLANES_WAVES))) void
k_section_planes(const TraceParams p, const PlaneParams x) {
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
        const float pt[3] = {r0.x, r0.y, r0.z}, nr[3] = {r1.x, r1.y, r1.z};
        const bool valid = finite3(v3(r0.x, r0.y, r0.z)) && finite3(v3(r1.x, r1.y, r1.z)) &&
                           !(r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f);
        __builtin_amdgcn_s_setprio(0);
        uint32_t found = 0;
        if (valid) {
            uint32_t* ids = nullptr;
            float4* segs = nullptr;
            uint32_t cap = 0;
            if (MODE == BM_PLANES_LIST) {
                const uint32_t o0 = p.q_ent[sidx], o1 = p.q_ent[sidx + 1];
                ids = p.q_counts ? p.q_counts + o0 : nullptr;
                segs = x.segs ? x.segs + 2 * (size_t)o0 : nullptr;
                cap = o1 > o0 ? o1 - o0 : 0u;
            }
            quad_section<COUNT, PRIO, MODE>(p, x, st, c, pt, nr, sidx, ids, segs, cap, found, cn, ct, maxsp);
            if (COUNT && c == 0) ch += MODE == BM_PLANES_ANY ? (found ? 1u : 0u) : found;
        }
        if (c == 0) {
            if (MODE == BM_PLANES_ANY) reinterpret_cast<uint8_t*>(p.q_out)[sidx] = found ? 1 : 0;
            else if (MODE == BM_PLANES_COUNT || p.q_out) reinterpret_cast<uint32_t*>(p.q_out)[sidx] = found;
        }
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

// launch_persistent with the second argument: min(p.persistent_blocks, the kernel's resident blocks)
template <typename K>
void launch_planes(K kernel, const TraceParams& p, const PlaneParams& x, hipStream_t s) {
    const uint32_t g = std::min(p.persistent_blocks, resident_blocks(kernel, BLOCK));
    kernel<<<g, BLOCK, 0, s>>>(p, x);
}

template <uint32_t MODE>
void launch_mode(const TraceParams& p, const PlaneParams& x, bool count, hipStream_t s) {
    if (count) launch_planes(k_section_planes<true, 1, MODE>, p, x, s);
    else if (p.prio_after == 0) launch_planes(k_section_planes<false, 0, MODE>, p, x, s);
    else launch_planes(k_section_planes<false, 1, MODE>, p, x, s);
}

}  // namespace

hipError_t launch_section_planes(const TraceParams& p, const PlaneParams& x, uint32_t mode, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_PLANES_LIST || (mode != BM_PLANES_LIST && !p.q_out) ||
        (mode == BM_PLANES_LIST && (!p.q_ent || (!p.q_counts && !x.segs))) || (p.num_tris && !x.meshes))
        return hipErrorInvalidValue;
    if (mode == BM_PLANES_COUNT) launch_mode<BM_PLANES_COUNT>(p, x, count, s);
    else if (mode == BM_PLANES_ANY) launch_mode<BM_PLANES_ANY>(p, x, count, s);
    else launch_mode<BM_PLANES_LIST>(p, x, count, s);
    return hipGetLastError();
}

}  // namespace bm
