// bm_trace_lanes.h — one lane per pixel: the single-lane BVH2 / BVH4 traversal (trace_pixel, shadow_ray)
// and its persistent kernel. Shared pieces: bm_trace_dev.h.
#pragma once
#include "bm_trace_dev.h"

namespace bm {
namespace {

// BVH4 node step (128-B record, SoA child boxes): slab-test the four children against [.., tmax],
// return the nearest hit child and push the other hit children farthest first, so they pop nearest
// first. The order is that of the children's order keys (bm_common.h), as in the oracle's
// visit_node, so the traversal (and the COUNT build's counters) match it step for step.
template <typename STACK>
__device__ __forceinline__ uint32_t visit4(const TraceParams& p, uint32_t node, const vec3f o, const vec3f inv,
                                           float tmax, STACK& st, int& sp) {
    const uint4* nd = p.nodes + 8 * (size_t)node;
    const uint4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5], rf = nd[6];
    const uint32_t LX[4] = {lx.x, lx.y, lx.z, lx.w}, LY[4] = {ly.x, ly.y, ly.z, ly.w}, LZ[4] = {lz.x, lz.y, lz.z, lz.w};
    const uint32_t HX[4] = {hx.x, hx.y, hx.z, hx.w}, HY[4] = {hy.x, hy.y, hy.z, hy.w}, HZ[4] = {hz.x, hz.y, hz.z, hz.w};
    const uint32_t R[4] = {rf.x, rf.y, rf.z, rf.w};
    // branch-free: every test below is a compare + mask, no short-circuit control flow
    // slab distances two children at a time: float2 lanes map onto gfx950's packed f32 add/mul
    // (v_pk_add_f32, v_pk_mul_f32), each element still one IEEE operation
    float tn[4];
    bool h[4];
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    const f32x2 ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
        const f32x2 tlx = (f32x2{u2f(LX[c]), u2f(LX[c + 1])} - ox) * ix, thx = (f32x2{u2f(HX[c]), u2f(HX[c + 1])} - ox) * ix;
        const f32x2 tly = (f32x2{u2f(LY[c]), u2f(LY[c + 1])} - oy) * iy, thy = (f32x2{u2f(HY[c]), u2f(HY[c + 1])} - oy) * iy;
        const f32x2 tlz = (f32x2{u2f(LZ[c]), u2f(LZ[c + 1])} - oz) * iz, thz = (f32x2{u2f(HZ[c]), u2f(HZ[c + 1])} - oz) * iz;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            tn[c + k] = fmaxf(fmaxf(fminf(tlx[k], thx[k]), fminf(tly[k], thy[k])), fminf(tlz[k], thz[k]));
            const float tf = fminf(fminf(fmaxf(tlx[k], thx[k]), fmaxf(tly[k], thy[k])), fmaxf(tlz[k], thz[k]));
            h[c + k] = (tn[c + k] <= tf) & (tf >= 0.0f) & (tn[c + k] <= tmax);
        }
    }
    // rank = position in the order of the hit children's keys (order_key; a miss is ~0u)
    uint32_t key[4], rank[4], nh = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        key[c] = h[c] ? order_key(tn[c], (uint32_t)c) : ~0u;
        nh += h[c] ? 1u : 0u;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint32_t r = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (d != c) r += key[d] < key[c] ? 1u : 0u;
        rank[c] = r;
    }
#pragma unroll
    for (uint32_t r = 3; r >= 1; --r) {
        uint32_t ref = EMPTY_REF;
        float t = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool sel = h[c] & (rank[c] == r);
            ref = sel ? R[c] : ref;
            t = sel ? tn[c] : t;
        }
        if (r < nh) {
            st.put(sp, ref, t);
            ++sp;
        }
    }
    uint32_t next = EMPTY_REF;
#pragma unroll
    for (int c = 0; c < 4; ++c) next = (h[c] & (rank[c] == 0)) ? R[c] : next;
    return next;
}

// Any-hit shadow segment o + s*d, 0 < s < 1 (oracle/beam_oracle.c orc_bvh_shadow, same traversal
// order, so the COUNT build's counters match). Boxes are culled beyond s = 1.
template <bool COUNT, typename STACK, uint32_t PRIO_AFTER, int W>
__device__ __forceinline__ bool shadow_ray(const TraceParams& p, STACK& st, const vec3f o, const vec3f d,
                                           unsigned long long& c_nodes, unsigned long long& c_tris) {
    const vec3f inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
    int sp = 0;
    uint32_t next = 0, iter = 0;
    for (;;) {
        prio_boost<PRIO_AFTER>(p, iter);
        if (next == EMPTY_REF) {
            if (sp == 0) return false;
            --sp;
            float tt;
            st.get(sp, next, tt);
        }
        if (next & LEAF_BIT) {
            const uint32_t first = next & FIRST_MASK, last = first + ((next >> 27) & 15u);
            float4 a = p.tris[3 * first + 0], b = p.tris[3 * first + 1], c = p.tris[3 * first + 2];
            for (uint32_t k = first;; ++k) {
                float4 na = a, nb = b, nc = c;
                if (k < last) {
                    na = p.tris[3 * k + 3];
                    nb = p.tris[3 * k + 4];
                    nc = p.tris[3 * k + 5];
                }
                if (COUNT) ++c_tris;
                float t, u, v;
                if (tri_test(a, b, c, o, d, t, u, v) && t > 0.0f && t < 1.0f) return true;
                if (k >= last) break;
                a = na;
                b = nb;
                c = nc;
            }
            next = EMPTY_REF;
            continue;
        }
        if (COUNT) ++c_nodes;
        if constexpr (W == 4) {
            next = visit4(p, next, o, inv, 1.0f, st, sp);
            continue;
        }
        const uint4* nd = p.nodes + 4 * (size_t)next;
        const uint4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        const float lo0[3] = {u2f(q0.x), u2f(q0.y), u2f(q0.z)}, hi0[3] = {u2f(q0.w), u2f(q1.x), u2f(q1.y)};
        const float lo1[3] = {u2f(q1.z), u2f(q1.w), u2f(q2.x)}, hi1[3] = {u2f(q2.y), u2f(q2.z), u2f(q2.w)};
        float tn0, tn1;
        const bool h0 = child_hit(lo0, hi0, o, inv, 1.0f, tn0);
        const bool h1 = child_hit(lo1, hi1, o, inv, 1.0f, tn1);
        if (h0 && h1) {
            const bool swap = tn1 < tn0;
            st.put(sp, swap ? q3.x : q3.y, 0.0f);
            ++sp;
            next = swap ? q3.y : q3.x;
        } else if (h0) {
            next = q3.x;
        } else if (h1) {
            next = q3.y;
        } else {
            next = EMPTY_REF;
        }
    }
}

// Trace one pixel (x, local row lr, global row gy) and write its framebuffer entries; returns hit.
template <bool COUNT, typename STACK, uint32_t PRIO_AFTER = 0, int SH = SH_NONE, int W = 2>
__device__ __forceinline__ bool trace_pixel(const TraceParams& p, STACK& st, uint32_t x, uint32_t lr, uint32_t gy,
                                            unsigned long long& c_nodes, unsigned long long& c_tris,
                                            unsigned long long& c_hits, unsigned long long (&c_sh)[3]) {
    const vec3f dir = primary_dir(p, x, gy);
    const vec3f inv = v3(1.f / dir.x, 1.f / dir.y, 1.f / dir.z);
    const vec3f eye = v3(p.eye[0], p.eye[1], p.eye[2]);

    float tbest = __builtin_inff(), bu = 0.f, bv = 0.f;
    uint32_t ibest = NO_TRI;
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
    if (COUNT && !p.num_tris) ++c_nodes;  // an empty scene: the all-empty root record orc_bvh_trace visits
    uint32_t iter = 0;

    for (;;) {
        prio_boost<PRIO_AFTER>(p, iter);
        if (next == EMPTY_REF) {
            // pop until an entry that can still hold a closer hit
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
        }
        if (next & LEAF_BIT) {
            const uint32_t first = next & FIRST_MASK, last = first + ((next >> 27) & 15u);
            // software-pipelined: the next triangle's record is in flight while this one is tested
            float4 a = p.tris[3 * first + 0], b = p.tris[3 * first + 1], c = p.tris[3 * first + 2];
            for (uint32_t k = first;; ++k) {
                float4 na = a, nb = b, nc = c;
                if (k < last) {
                    na = p.tris[3 * k + 3];
                    nb = p.tris[3 * k + 4];
                    nc = p.tris[3 * k + 5];
                }
                if (COUNT) ++c_tris;
                // bmTriIntersect as in tri_test, written out: this form schedules better here
                const vec3f e1 = v3(b.x, b.y, b.z), e2 = v3(c.x, c.y, c.z);
                const vec3f pv = cross(dir, e2);
                const float det = dot(e1, pv);
                const vec3f tv = sub(eye, v3(a.x, a.y, a.z));
                const float un = dot(tv, pv);
                const vec3f qv = cross(tv, e1);
                const float vn = dot(dir, qv);
                const float ra = __builtin_amdgcn_rcpf(det);
                const float ua = un * ra, va = vn * ra;
                const bool far_out =
                    fabsf(det) >= 0x1p-100f &&
                    (ua < -0x1p-10f || ua > 1.0f + 0x1p-10f || va < -0x1p-10f || va + ua > 1.0f + 0x1p-9f);
                if (!far_out) {
                    const float idet = 1.f / det;
                    const float u = un * idet;
                    const float v = vn * idet;
                    if (!(u < 0 || u > 1) && !(v < 0 || v + u > 1)) {
                        const float t = dot(e2, qv) * idet;
                        const uint32_t id = f2u(a.w);
                        if (t > 0.0f && t < 3.40282347e+38f && (t < tbest || (t == tbest && id < ibest))) {
                            tbest = t;
                            ibest = id;
                            bu = u;
                            bv = v;
                        }
                    }
                }
                if (k >= last) break;
                a = na;
                b = nb;
                c = nc;
            }
            next = EMPTY_REF;
            continue;
        }
        if constexpr (W == 4) {
            if (COUNT) ++c_nodes;
            next = visit4(p, next, eye, inv, tbest, st, sp);
            continue;
        }
        const uint4* nd = p.nodes + 4 * (size_t)next;
        const uint4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
        if (COUNT) ++c_nodes;
        const float lo0[3] = {u2f(q0.x), u2f(q0.y), u2f(q0.z)}, hi0[3] = {u2f(q0.w), u2f(q1.x), u2f(q1.y)};
        const float lo1[3] = {u2f(q1.z), u2f(q1.w), u2f(q2.x)}, hi1[3] = {u2f(q2.y), u2f(q2.z), u2f(q2.w)};
        float tn0, tn1;
        const bool h0 = child_hit(lo0, hi0, eye, inv, tbest, tn0);
        const bool h1 = child_hit(lo1, hi1, eye, inv, tbest, tn1);
        if (h0 && h1) {
            const bool swap = tn1 < tn0;
            st.put(sp, swap ? q3.x : q3.y, swap ? tn0 : tn1);
            ++sp;
            next = swap ? q3.y : q3.x;
        } else if (h0) {
            next = q3.x;
        } else if (h1) {
            next = q3.y;
        } else {
            next = EMPTY_REF;
        }
    }

    const size_t o = (size_t)lr * p.width + x;
    uint32_t packed = MISS_PACKED;
    float nzv = 0.0f;
    if (ibest != NO_TRI) {
        packed = shade_hit(p, ibest, bu, bv, nzv);
        if (COUNT) ++c_hits;
    }
    p.packed[(size_t)lr * p.pitch_u32 + x] = packed;
    p.tri_id[o] = ibest;
    p.t[o] = tbest;
    if (p.nz) p.nz[o] = nzv;
    if (SH == SH_QUEUE) p.shadow[o] = 0;
    if (SH == SH_FUSED) {
        bool occ = false;
        if (ibest != NO_TRI) {
            vec3f so, sd;
            shadow_segment(p, eye, dir, tbest, so, sd);
            occ = shadow_ray<COUNT, STACK, PRIO_AFTER, W>(p, st, so, sd, c_sh[0], c_sh[1]);
            if (COUNT) c_sh[2] += occ;
        }
        p.shadow[o] = occ ? 1 : 0;
    }
    return ibest != NO_TRI;
}

// Shadow pass input: the hit pixels of a wave are appended to the queue with one atomic per wave
// (ballot + popcount ranks). Queue order varies run to run; each entry's result does not.
__device__ __forceinline__ void enqueue_hit(const TraceParams& p, bool hit, uint32_t pix) {
    const unsigned long long hits = ballot(hit);
    if (!hits) return;
    const int leader = __ffsll((long long)ballot(1)) - 1;
    const uint32_t lane = __lane_id();
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(p.queue_count, (uint32_t)__popcll(hits));
    base = __shfl(base, leader);
    if (hit) p.queue[base + __popcll(hits & ((1ull << lane) - 1ull))] = pix;
}

// Persistent grid: wave g traces 8x8 tiles g, g + G, g + 2G, ... (G = waves in the grid).
// Dynamic tile scheduling: the wave's next 8x8 tile from the context's ticket counter (one atomic
// per tile). Tickets past the frame's tiles end the wave, so a launch consumes exactly
// tiles + waves tickets and the host advances tile_base by that much.
__device__ __forceinline__ uint32_t next_tile(const TraceParams& p) {
    uint32_t t = 0;
    if (__lane_id() == 0) t = (uint32_t)(atomicAdd(p.tile_ctr, 1ull) - p.tile_base);
    return __builtin_amdgcn_readfirstlane(t);
}

// DIAG: see diag_wave_record.
template <bool COUNT, int LDS_N, int OVF, uint32_t PRIO = 0, int SH = SH_NONE, int W = 2, bool DYN = false,
          bool DIAG = false>
__global__ __launch_bounds__(BLOCK) BM_TRACE_OCCUPANCY void k_trace_persistent(const TraceParams p) {
    static_assert(!DIAG || COUNT, "the diagnostic build counts work");
    const uint64_t t_start = DIAG ? __builtin_amdgcn_s_memrealtime() : 0;
    uint32_t diag_work = 0;
    __shared__ uint32_t s_ref[LDS_N][BLOCK];
    __shared__ float s_t[LDS_N][BLOCK];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    Stack<LDS_N, OVF> st;
    st.s_ref = s_ref;
    st.s_t = s_t;
    st.tid = tid;
    const uint32_t slot = blockIdx.x * BLOCK + tid;
    st.g_ref = p.ovf_ref + slot;
    st.g_t = p.ovf_t + slot;
    st.stride = p.ovf_stride;
    const uint32_t tiles_x = (p.width + 7) / 8, tiles_y = (p.local_rows + 7) / 8;
    const uint32_t ntiles = tiles_x * tiles_y;
    const uint32_t nwaves = gridDim.x * WAVES;
    unsigned long long cn = 0, ct = 0, ch = 0, csh[3] = {0, 0, 0};
    for (uint32_t i = DYN ? next_tile(p) : blockIdx.x * WAVES + w; i < ntiles;
         i = DYN ? next_tile(p) : i + nwaves) {
        // scramble: tile = i * P mod ntiles (P prime > ntiles: a bijection) spreads the costly
        // tiles of a compact subject evenly over waves, SIMDs and CUs
        const uint32_t t = p.scramble ? (uint32_t)(((uint64_t)i * 2654435761ull) % ntiles) : i;
        const uint32_t x = (t % tiles_x) * 8 + (lane & 7);
        const uint32_t lr = (t / tiles_x) * 8 + (lane >> 3);
        const uint32_t gy = lr < p.local_rows ? global_row(p, lr) : p.height;
        const unsigned long long before = cn + ct;
        if (x < p.width && gy < p.height) {
            __builtin_amdgcn_s_setprio(0);
            const bool hit = trace_pixel<COUNT, decltype(st), PRIO, SH, W>(p, st, x, lr, gy, cn, ct, ch, csh);
            if (SH == SH_QUEUE) enqueue_hit(p, hit, lr * p.width + x);
        }
        if (DIAG) diag_add_tile(diag_work, cn + ct - before);
    }
    flush_counters<COUNT>(p, cn, ct, ch, csh);
    if (DIAG) diag_wave_record(p, w, lane, t_start, diag_work);
}

}  // namespace
}  // namespace bm
