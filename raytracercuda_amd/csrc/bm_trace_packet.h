// bm_trace_packet.h — wave packets: one 8x8 tile of coherent primary rays per wave over the BVH4
// (k_trace_packet). Shared pieces: bm_trace_dev.h.
#pragma once
#include "bm_trace_dev.h"

namespace bm {
namespace {

// ---- wave packets: one 8x8 tile of coherent primary rays per wave over the BVH4 (TRACE_PACKET) ------
// the quad step is bound by its dependent chain (LDS pop -> seven per-lane record loads ->
// slab tests -> DPP ranking -> LDS push, ~1,800 cycles) and the filled view takes ~16.6 of them per ray.
// Here the traversal state is the wave's, not the lane's: one node record per wave step, read by
// scalar loads (the record address is wave-uniform: the constant address space makes the compiler
// issue s_load into SGPRs), each lane slab-tests the four children against its own ray, a ballot per
// child gives the lanes that descend, and the wave walks one shared stack in LDS whose entries carry
// (child box, child ref, lane mask). A popped entry's lanes re-test its box against their current
// closest hit, so a subtree is entered only by lanes whose own traversal would enter it; every lane
// keeps its own (t, id) closest hit with lowest-id ties, which does not depend on the order the
// subtrees are visited in — the frame equals the oracle's (the visit order and the COUNT counters do
// not, so counting traces keep the quad kernel). That holds where the box prune is conservative: for
// eyes within 32 scene extents of the scene. Farther out a box that holds a ray's
// closest hit can fail tn <= tbest by rounding, whether it does depends on what was found before it,
// and a packet visits in its first lane's order (measured at 4096 extents: on a pixel or two of a frame
// it kept the hit brute force finds where the per-ray order loses it). So the host launches packets for
// eyes within that distance only and the quad kernel beyond (bm_api.cpp eye_in_envelope). Children are
// ordered by the entry distances of the packet's first lane (children that lane misses after).
// Stack bound: the BVH4 levels of a < 64-level Karras tree are < 32, a packet step pushes <= 3
// siblings, and the stack holds siblings of the current path only: PK_DEPTH = MAX_STACK entries.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const u32x4 cuint4;   // scalar (SMEM) loads of uniform records
typedef __attribute__((address_space(4))) const uint32_t cuint;
typedef unsigned long long u64x4 __attribute__((ext_vector_type(4)));
constexpr int PK_DEPTH = MAX_STACK;
constexpr int PACKET_WAVES = 8;  // waves per SIMD the packet kernel's registers must allow (6 / 7: 1-2 % slower, r06_v11)
// The walk's form, each choice measured against its alternative (whose code is not kept):
//  - stack entries are 16 B and a pop re-loads the child's box from its parent's record by scalar
//    loads (filled view 333 -> 314 us against the box in LDS beside the entry);
//  - a pushed child carries its parent node's lanes M instead of the child's own mask B and no ref
//    (read from the parent's record at the pop). The pop re-tests the child's box for the lanes it
//    carries against their closest hit then (t_pop <= t_push): M & test(t_pop) = B & test(t_pop),
//    since B = M & test(t_push) and the box terms are the same arithmetic on the same operands. No
//    per-push picks;
//  - child and pop masks are ANDs of per-compare ballots (scalar); the children's order keys are
//    formed per lane by VALU and the lead lane's read (scalar key forms cost SALU);
//  - the children are ordered by the packet's first lane's entry distances and ranked by a scalar
//    sorting network (per-child compare counts: 4-5 % slower in flight), then picked by slot from
//    SGPR vectors;
//  - the node is never passed through readfirstlane at the loop head (every assignment is uniform);
//  - leaf triangle records are loaded one at a time, each before its test;
//  - a packet keeps its issue priority throughout.

// Slab planes by direction sign. When every ray of the tile has finite, nonzero inverse
// direction components of one sign per axis (all tiles but those on the image's sign-change lines),
// the entry plane of each axis is the same for all of them: lo for a positive component, hi for a
// negative one. Then min(t_lo, t_hi) is t_near exactly — (b - o) * inv is monotone in b for a finite
// inv of fixed sign, so t_lo <= t_hi or the reverse, ties included (a signed zero only ties) — and
// t_far likewise, and NaN-box (empty) slots give NaN either way: tn = max3 of the near values and
// tf = min3 of the far ones, bit-identical to the min/max form, two operations per child instead of
// eight. The walk is instantiated per sign combination (SG = x | y << 1 | z << 2 negative), SG = 8 the
// general form for the other tiles.

struct PkHit {
    float t, u, v;
    uint32_t id;
};

// One 8x8 tile's walk by one wave (all 64 lanes, wave-uniform control flow). s_e: the wave's stack (PK_DEPTH).
template <bool DIAG, int SG>
__device__ __forceinline__ void packet_walk(const TraceParams& p, int lane, uint4* __restrict__ s_e,
                                            unsigned long long* __restrict__ dslot, uint64_t t_start, bool valid,
                                            const vec3f eye, const vec3f dir, const vec3f inv, PkHit& hit) {
    uint32_t d_nodes = 0, d_leaves = 0, d_tris = 0, d_lanes = 0;
    (void)dslot;
    constexpr bool NX = SG & 1, NY = SG & 2, NZ = SG & 4;  // (SG < 8) axes whose entry plane is hi
    // the eye pairs held in VGPRs (a packed op takes one SGPR operand: the record's)
    f32x2 ox = {eye.x, eye.x}, oy = {eye.y, eye.y}, oz = {eye.z, eye.z};
    asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz));
    const f32x2 ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
    float tbest = __builtin_inff(), bu = 0.f, bv = 0.f;
    uint32_t ibest = NO_TRI;
    unsigned long long M = ballot(valid);  // lanes of the current node
    uint32_t node = p.num_tris && M ? 0u : EMPTY_REF;
    int sp = 0;
    cuint4* const nodes = (cuint4*)(p.nodes);  // generic -> constant address space (a C cast)
    cuint4* const tris = (cuint4*)(p.tris);
    for (;;) {
        if (node != EMPTY_REF) {
            const bool act = (M >> lane) & 1ull;
            if (node & LEAF_BIT) {
                const uint32_t first = node & FIRST_MASK, cnt = ((node >> 27) & 15u) + 1u;
                if (DIAG) ++d_leaves, d_tris += cnt;
                // leaf triangle records loaded per batch before their tests (one; written as a plain
                // loop over the records the compiler generates other, longer code)
                constexpr uint32_t LB = 1;
                for (uint32_t k0 = 0; k0 < cnt; k0 += LB) {  // LB records in flight, then their tests
                    u32x4 r[LB][3];
#pragma unroll
                    for (uint32_t j = 0; j < LB; ++j) {
                        cuint4* tr = tris + 3 * (size_t)(first + min(k0 + j, cnt - 1u));
                        r[j][0] = tr[0], r[j][1] = tr[1], r[j][2] = tr[2];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < LB; ++j) {
                        if (k0 + j < cnt && act) {
                            float tt, uu, vv;
                            const float4 a = make_float4(u2f(r[j][0].x), u2f(r[j][0].y), u2f(r[j][0].z), 0.f);
                            const float4 b = make_float4(u2f(r[j][1].x), u2f(r[j][1].y), u2f(r[j][1].z), 0.f);
                            const float4 c = make_float4(u2f(r[j][2].x), u2f(r[j][2].y), u2f(r[j][2].z), 0.f);
                            if (tri_test(a, b, c, eye, dir, tt, uu, vv) && tt > 0.0f && tt < 3.40282347e+38f) {
                                const uint32_t id = r[j][0].w;
                                if (tt < tbest || (tt == tbest && id < ibest)) {
                                    tbest = tt;
                                    ibest = id;
                                    bu = uu;
                                    bv = vv;
                                }
                            }
                        }
                    }
                }
                node = EMPTY_REF;
            } else {
                if (DIAG) ++d_nodes, d_lanes += (uint32_t)__popcll(M);
                cuint4* nd = nodes + 8 * (size_t)node;
                const u32x4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5], rf = nd[6];
                const uint32_t LX[4] = {lx.x, lx.y, lx.z, lx.w}, LY[4] = {ly.x, ly.y, ly.z, ly.w};
                const uint32_t LZ[4] = {lz.x, lz.y, lz.z, lz.w}, HX[4] = {hx.x, hx.y, hx.z, hx.w};
                const uint32_t HY[4] = {hy.x, hy.y, hy.z, hy.w}, HZ[4] = {hz.x, hz.y, hz.z, hz.w};
                // slab tests two children at a time (adjacent SGPRs feed the packed f32 operations)
                unsigned long long B[4];
                uint32_t kl[4];  // this lane's order key of each child (its misses after its hits)
#pragma unroll
                for (int c = 0; c < 4; c += 2) {
                    const f32x2 tlx = (f32x2{u2f(LX[c]), u2f(LX[c + 1])} - ox) * ix;
                    const f32x2 thx = (f32x2{u2f(HX[c]), u2f(HX[c + 1])} - ox) * ix;
                    const f32x2 tly = (f32x2{u2f(LY[c]), u2f(LY[c + 1])} - oy) * iy;
                    const f32x2 thy = (f32x2{u2f(HY[c]), u2f(HY[c + 1])} - oy) * iy;
                    const f32x2 tlz = (f32x2{u2f(LZ[c]), u2f(LZ[c + 1])} - oz) * iz;
                    const f32x2 thz = (f32x2{u2f(HZ[c]), u2f(HZ[c + 1])} - oz) * iz;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        float tn, tf;
                        if constexpr (SG < 8) {  // entry / exit planes known per axis
                            tn = fmaxf(fmaxf(NX ? thx[k] : tlx[k], NY ? thy[k] : tly[k]), NZ ? thz[k] : tlz[k]);
                            tf = fminf(fminf(NX ? tlx[k] : thx[k], NY ? tly[k] : thy[k]), NZ ? tlz[k] : thz[k]);
                        } else {
                            tn = fmaxf(fmaxf(fminf(tlx[k], thx[k]), fminf(tly[k], thy[k])), fminf(tlz[k], thz[k]));
                            tf = fminf(fminf(fmaxf(tlx[k], thx[k]), fmaxf(tly[k], thy[k])), fmaxf(tlz[k], thz[k]));
                        }
                        // each compare's ballot is its own SGPR mask; the node's lanes and the AND are scalar
                        const bool c1 = tn <= tf, c2 = tf >= 0.0f, c3 = tn <= tbest;
                        B[c + k] = ballot(c1) & ballot(c2) & ballot(c3) & M;
                        // every lane's key by VALU (the lead lane's is read below): fewer scalar operations
                        kl[c + k] = (c1 & c2 & c3) ? order_key(tn, (uint32_t)(c + k)) : (0xFFFFFFF0u | (uint32_t)(c + k));
                    }
                }
                // order by the packet's first lane; a child no lane enters ranks last
                const int lead = __builtin_ctzll(M);
                uint32_t K[4];
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    // sortable as they are: a child no lane enters is 0xFFFFFFFC | slot
                    K[c] = B[c] ? (uint32_t)__builtin_amdgcn_readlane((int)kl[c], lead) : (0xFFFFFFFCu | (uint32_t)c);
                node = EMPTY_REF;
                unsigned long long Mn = 0;
                {  // keys sorted by a five-exchange network (scalar min/max; a key's low two bits are its slot,
                   // a child no lane enters sorts last as ~0 - 3 + slot), then the children by rank
                    uint32_t k0 = K[0], k1 = K[1], k2 = K[2], k3 = K[3];
                    auto cx = [](uint32_t& x, uint32_t& y) {
                        const uint32_t lo = min(x, y), hi = max(x, y);
                        x = lo, y = hi;
                    };
                    cx(k0, k1), cx(k2, k3), cx(k0, k2), cx(k1, k3), cx(k1, k2);
                    const uint32_t ks[4] = {k0, k1, k2, k3};
                    const uint32_t pcs = (uint32_t)((nd - nodes) >> 3) << 2;
                    // dynamic element of an SGPR vector (s_movrels) instead of a branch chain
                    const u64x4 BV = {B[0], B[1], B[2], B[3]};
                    auto pick_r = [&](uint32_t sl) { return rf[sl & 3u]; };
                    auto pick_b = [&](uint32_t sl) { return BV[sl & 3u]; };
                    // a key below 0xFFFFFFFC is a child some lane enters (no count of them needed: the
                    // pushes go farthest first, each on top of the last, so they pop nearest first)
                    if (k0 < 0xFFFFFFFCu) {
                        node = pick_r(k0 & 3u);
                        Mn = pick_b(k0 & 3u);
                    }
#pragma unroll
                    for (int r = 3; r >= 1; --r) {
                        if (ks[r] < 0xFFFFFFFCu) {
                            const uint32_t sl = ks[r] & 3u;
                            // the node's lanes: the pop's re-test leaves exactly the child's (see above)
                            const int at = __builtin_amdgcn_readfirstlane(min(sp, PK_DEPTH - 1));
                            if (lane == 0) s_e[at] = make_uint4(0u, (uint32_t)M, (uint32_t)(M >> 32), pcs | sl);
                            sp = __builtin_amdgcn_readfirstlane(min(sp + 1, PK_DEPTH));
                        }
                    }
                    sp = __builtin_amdgcn_readfirstlane(sp);  // uniform (the lane-0 stores must not make it look divergent)
                }
                M = Mn;
                continue;
            }
        }
        // pop: the next entry some lane still enters (its box re-tested against the lane's closest hit)
        bool found = false;
        while (sp > 0) {
            --sp;
            const uint4 e = s_e[sp];
            const uint32_t pcs = __builtin_amdgcn_readfirstlane(e.w);
            const unsigned long long em = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane(e.z) << 32) |
                                          (uint32_t)__builtin_amdgcn_readfirstlane(e.y);
            cuint* pr = (cuint*)(p.nodes) + 32 * (size_t)(pcs >> 2) + (pcs & 3u);
            const float blx = u2f(pr[0]), bly = u2f(pr[4]), blz = u2f(pr[8]);
            const float bhx = u2f(pr[12]), bhy = u2f(pr[16]), bhz = u2f(pr[20]);
            const uint32_t eref = pr[24];  // the child's ref from its parent's record
            const f32x2 tx = (f32x2{blx, bhx} - ox) * ix, ty = (f32x2{bly, bhy} - oy) * iy, tz = (f32x2{blz, bhz} - oz) * iz;
            float tn, tf;
            if constexpr (SG < 8) {
                tn = fmaxf(fmaxf(NX ? tx.y : tx.x, NY ? ty.y : ty.x), NZ ? tz.y : tz.x);
                tf = fminf(fminf(NX ? tx.x : tx.y, NY ? ty.x : ty.y), NZ ? tz.x : tz.y);
            } else {
                tn = fmaxf(fmaxf(fminf(tx.x, tx.y), fminf(ty.x, ty.y)), fminf(tz.x, tz.y));
                tf = fminf(fminf(fmaxf(tx.x, tx.y), fmaxf(ty.x, ty.y)), fmaxf(tz.x, tz.y));
            }
            M = em & ballot(tn <= tf) & ballot(tf >= 0.0f) & ballot(tn <= tbest);
            if (M) {
                node = __builtin_amdgcn_readfirstlane(eref);
                found = true;
                break;
            }
        }
        if (!found) break;
    }
    if (DIAG && lane == 0) {  // per tile: start, end, (leaf << 32 | node steps), (tri tests << 32 | lanes)
        dslot[0] = t_start;
        dslot[1] = __builtin_amdgcn_s_memrealtime();
        dslot[2] = ((uint64_t)d_leaves << 32) | d_nodes;
        dslot[3] = ((uint64_t)d_tris << 32) | d_lanes;
    }
    hit = PkHit{tbest, bu, bv, ibest};
}

template <bool DIAG>
__device__ __forceinline__ void packet_tile(const TraceParams& p, uint32_t tile, uint32_t tiles_x, int lane,
                                            uint4* __restrict__ s_e, unsigned long long* __restrict__ dslot) {
    const uint64_t t_start = DIAG ? __builtin_amdgcn_s_memrealtime() : 0;
    const uint32_t x = (tile % tiles_x) * 8 + (lane & 7);
    const uint32_t lr = (tile / tiles_x) * 8 + (lane >> 3);
    const uint32_t gy = lr < p.local_rows ? global_row(p, lr) : p.height;
    const bool valid = x < p.width && gy < p.height;
    const vec3f eye = v3(p.eye[0], p.eye[1], p.eye[2]);
    vec3f dir = v3(0.f, 0.f, 1.f), inv = v3(0.f, 0.f, 1.f);
    if (valid) {
        dir = primary_dir(p, x, gy);
        inv = v3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
    }
    PkHit hit;
    // the tile's sign combination when its rays' inverse components are finite and of one sign per axis
    const unsigned long long V = ballot(valid);
    const bool fin = __builtin_isfinite(inv.x) && __builtin_isfinite(inv.y) && __builtin_isfinite(inv.z);
    const unsigned long long bad = V & ~ballot(fin);
    const unsigned long long nx = ballot(valid && inv.x < 0.f), ny = ballot(valid && inv.y < 0.f),
                             nz = ballot(valid && inv.z < 0.f);
    const bool uni = !bad && (nx == 0 || nx == V) && (ny == 0 || ny == V) && (nz == 0 || nz == V);
    const int sg = uni ? (nx ? 1 : 0) | (ny ? 2 : 0) | (nz ? 4 : 0) : 8;
    switch (sg) {
        case 0: packet_walk<DIAG, 0>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 1: packet_walk<DIAG, 1>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 2: packet_walk<DIAG, 2>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 3: packet_walk<DIAG, 3>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 4: packet_walk<DIAG, 4>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 5: packet_walk<DIAG, 5>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 6: packet_walk<DIAG, 6>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        case 7: packet_walk<DIAG, 7>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
        default: packet_walk<DIAG, 8>(p, lane, s_e, dslot, t_start, valid, eye, dir, inv, hit); break;
    }
    if (!valid) return;
    const uint32_t o32 = lr * p.width + x;
    uint32_t packed = MISS_PACKED;
    float nzv = 0.0f;
    if (hit.id != NO_TRI) packed = shade_hit(p, hit.id, hit.u, hit.v, nzv);
    p.packed[(size_t)lr * p.pitch_u32 + x] = packed;
    p.tri_id[o32] = hit.id;
    p.t[o32] = hit.t;
    if (p.nz) p.nz[o32] = nzv;
}


// Tile order: one tile per wave in screen order (grid = tiles / 4 blocks; the hardware dispatcher
// balances). A persistent grid whose block b owns the tiles b, b + B, ... (B = blocks) and hands them
// to its four waves by an LDS ticket, longest first by the previous trace's tile costs (the quad
// kernel's cost-ordered schedule), was measured slower (filled view 302 -> 355 us, C4 284 -> 356) and
// is not kept: the driver loop cost the kernel 9 SGPRs and 39 spills, and the tiles it started first
// ran slower on cold caches.
template <int SH, bool DIAG = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(PACKET_WAVES))) void k_trace_packet(
    const TraceParams p) {
    static_assert(SH == SH_NONE, "packets: primary rays");
    __shared__ uint4 s_e[WAVES][PK_DEPTH];  // (0, node's lanes lo, lanes hi, parent << 2 | slot)
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tiles_x = (p.width + 7) / 8, tiles_y = (p.local_rows + 7) / 8;
    const uint32_t ntiles = tiles_x * tiles_y;
    const uint32_t tile = blockIdx.x * WAVES + (uint32_t)w;
    if (tile >= ntiles) return;
    packet_tile<DIAG>(p, tile, tiles_x, lane, s_e[w], DIAG ? p.diag + 4 * (size_t)tile : nullptr);
}

}  // namespace
}  // namespace bm
