// bm_sweep.hip — sphere-cast queries: for each sweep of a caller's batch in device memory (a ray record
// whose pad word is a radius), how far the sphere travels along the direction before it touches the scene,
// and where (bm_scene_sweep_spheres). The result is a bm_hit (t, u, v, tri_id) of the contact point, so
// bm_scene_hit_attributes turns it into the contact position, the normal there or the owning mesh and face.
//   k_sweep_spheres  persistent grid; a wave takes batches of 16 consecutive sweeps (512 contiguous
//                    bytes), lane 4q+c works for sweep 16b+q — the shape of k_query_rays
// The traversal (quad_sweep) is ordered by entry distance over the BVH4: lane c slab-tests the centre's
// line against child c's box moved outwards by radius + m (sweep_visit), the kept children are ranked by
// order_key and pushed farthest first with their entry distance as stack key, and a subtree is dropped when
// the line enters its padded box beyond the best t found so far. m makes that pruning conservative against
// the rounding of the triangle function, so the result is the lexicographic minimum of (t, id) over ALL
// triangles, bit for bit what an exhaustive evaluation of tri_sweep gives.
#include "bm_sweep_dev.h"

namespace bm {
namespace {

// First contact of one sweep over the quad: the lexicographic minimum of (t, id) over the triangles
// tri_sweep accepts with t <= best on entry (the sweep's tl). One iteration is quad_closest's: the pending
// leaf, the pop that follows it, the node visit. ANY: returns at the first accepted triangle (ibest is then
// that triangle's id, and nothing else of the result is meaningful). maxsp (COUNT): the most stack entries
// held at once.
template <bool COUNT, uint32_t PRIO, bool ANY, typename QS>
__device__ __forceinline__ void quad_sweep(const TraceParams& p, const QS& st, int c, const vec3f o, const vec3f d,
                                           const vec3f inv, float r, float pad, float tl, float& best,
                                           uint32_t& ibest, float& bu, float& bv, unsigned long long& cn,
                                           unsigned long long& ct, int& maxsp) {
    int sp = 0;
    uint32_t next = p.num_tris ? 0u : EMPTY_REF;
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
                    const float4 a = p.tris[3 * k + 0], b = p.tris[3 * k + 1], cc = p.tris[3 * k + 2];
                    float tt, uu, vv;
                    if (tri_sweep(a, b, cc, o, d, r, tl, tt, uu, vv)) t = tt, u = uu, v = vv, id = f2u(a.w);
                }
                quad_min_hit(t, id, u, v);
                if (t < best || (t == best && id < ibest)) {
                    best = t;
                    ibest = id;
                    bu = u;
                    bv = v;
                }
                if (COUNT && c == 0) ct += min(4u, cnt - k0);
                if (ANY && ibest != NO_TRI) return;
            }
            next = EMPTY_REF;
        }
        if (next == EMPTY_REF) {
            bool found = false;
            while (sp > 0) {
                --sp;
                uint32_t ref;
                float key;
                st.get(sp, ref, key);
                if (!(key > best)) {
                    next = ref;
                    found = true;
                    break;
                }
            }
            if (!found) break;
            if (next & LEAF_BIT) continue;  // a popped leaf: evaluated at the top of the next iteration
        }
        if (COUNT && c == 0) ++cn;
        next = sweep_visit(p, next, c, o, inv, pad, best, st, sp);
        if (COUNT) maxsp = max(maxsp, sp);
#pragma unroll
        for (int extra = 1; extra < QUAD_VISITS; ++extra) {
            if (next == EMPTY_REF || (next & LEAF_BIT)) break;
            if (COUNT && c == 0) ++cn;
            next = sweep_visit(p, next, c, o, inv, pad, best, st, sp);
            if (COUNT) maxsp = max(maxsp, sp);
        }
    }
}

constexpr int SWEEP_WAVES = 6;  // waves per SIMD the registers must allow: 78 VGPRs, the most without scratch

// A sweep record is two float4: (origin, tmax) (dir, radius). The four lanes of a quad load the same 32
// bytes. An invalid sweep (a non-finite origin or direction component, an all-zero direction, tmax NaN or
// negative, a radius that is NaN, infinite or <= 0) is finished here with the miss record, or 0, so no NaN
// reaches the traversal. The union of the root record's child boxes, which the margin is sized from, is read
// once per kernel (wave-uniform loads; empty slots are NaN: fminf and fmaxf skip them).
template <bool COUNT, uint32_t PRIO, bool ANY>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(COUNT ? 1 : SWEEP_WAVES))) void
k_sweep_spheres(const TraceParams p) {
    __shared__ uint2 s_stk[QUAD_LDS][QRAYS];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int c = lane & 3, q = lane >> 2;
    const QStack<QUAD_LDS> st = quad_stack<QUAD_LDS>(p, s_stk, w * 16 + q);
    unsigned long long cn = 0, ct = 0, ch = 0;
    const unsigned long long none[3] = {0, 0, 0};
    int maxsp = 0;
    const float nan = __builtin_nanf("");
    float ulo[3] = {nan, nan, nan}, uhi[3] = {nan, nan, nan};
    if (p.num_tris) {
        const uint4* rn = p.nodes;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 lo = rn[k], hi = rn[3 + k];
            ulo[k] = fminf(fminf(u2f(lo.x), u2f(lo.y)), fminf(u2f(lo.z), u2f(lo.w)));
            uhi[k] = fmaxf(fmaxf(u2f(hi.x), u2f(hi.y)), fmaxf(u2f(hi.z), u2f(hi.w)));
        }
    }
    const float root = fmaxf(fmaxf(fmaxf(fabsf(ulo[0]), fabsf(uhi[0])), fmaxf(fabsf(ulo[1]), fabsf(uhi[1]))),
                             fmaxf(fabsf(ulo[2]), fabsf(uhi[2])));
    const uint32_t n = p.q_n;
    const uint32_t nbatch = (n >> 4) + ((n & 15u) ? 1u : 0u), nwaves = gridDim.x * WAVES;
    for (uint32_t b = blockIdx.x * WAVES + w; b < nbatch; b += nwaves) {
        const uint32_t sidx = b * 16 + (uint32_t)q;
        if (sidx >= n) continue;  // the last batch: whole quads only
        const float4 r0 = p.q_rays[2 * (size_t)sidx], r1 = p.q_rays[2 * (size_t)sidx + 1];
        const vec3f o = v3(r0.x, r0.y, r0.z), d = v3(r1.x, r1.y, r1.z);
        const float tmax = r0.w, r = r1.w;
        const bool valid = finite3(o) && finite3(d) && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f) && tmax >= 0.0f &&
                           r > 0.0f && r < __builtin_inff();  // the comparisons are false for NaN
        __builtin_amdgcn_s_setprio(0);
        float best = __builtin_inff(), bu = 0.f, bv = 0.f;
        uint32_t ibest = NO_TRI;
        if (valid && p.num_tris) {
            const float tl = fminf(tmax, 3.40282347e+38f);
            const float rel = fmaxf(fmaxf(fmaxf(fabsf(o.x - ulo[0]), fabsf(uhi[0] - o.x)),
                                          fmaxf(fabsf(o.y - ulo[1]), fabsf(uhi[1] - o.y))),
                                    fmaxf(fabsf(o.z - ulo[2]), fabsf(uhi[2] - o.z)));
            const float big = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) + root;
            const float pad = r + sweep_margin(rel, r, big);
            const vec3f inv = v3(1.f / d.x, 1.f / d.y, 1.f / d.z);
            best = tl;
            quad_sweep<COUNT, PRIO, ANY>(p, st, c, o, d, inv, r, pad, tl, best, ibest, bu, bv, cn, ct, maxsp);
            if (COUNT && c == 0 && ibest != NO_TRI) ++ch;
        }
        if (ANY) {
            if (c == 0) reinterpret_cast<uint8_t*>(p.q_out)[sidx] = ibest != NO_TRI ? 1 : 0;
        } else {
            if (ibest == NO_TRI) best = __builtin_inff(), bu = 0.f, bv = 0.f;
            // the result record: one 16-B store by the quad's first lane, as k_query_rays
            if (c == 0) reinterpret_cast<float4*>(p.q_out)[sidx] = make_float4(best, bu, bv, u2f(ibest));
        }
    }
    flush_counters<COUNT>(p, cn, ct, ch, none);
    if (COUNT) atomicMax(&p.counters[3], (unsigned long long)maxsp);
}

template <bool ANY>
void launch_mode(const TraceParams& p, bool count, hipStream_t s) {
    if (count) launch_persistent(k_sweep_spheres<true, 1, ANY>, p, s, nullptr);
    else if (p.prio_after == 0) launch_persistent(k_sweep_spheres<false, 0, ANY>, p, s, nullptr);
    else launch_persistent(k_sweep_spheres<false, 1, ANY>, p, s, nullptr);
}

}  // namespace

hipError_t launch_sweep_spheres(const TraceParams& p, uint32_t mode, bool count, hipStream_t s) {
    if (p.q_n == 0) return hipSuccess;
    if (p.bvh_width != 4 || mode > BM_SWEEP_ANY) return hipErrorInvalidValue;
    if (mode == BM_SWEEP_CLOSEST) launch_mode<false>(p, count, s);
    else launch_mode<true>(p, count, s);
    return hipGetLastError();
}

}  // namespace bm
