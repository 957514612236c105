// bm_trace_dev.h — what the device code of every trace kernel family shares: the persistent launch,
// the single-lane stack, the ray set-up, shading, counters and the DIAG record. The families are in
// bm_trace_lanes.h (one lane per pixel), bm_trace_quad.h (ray quads, cull + compacted rays) and
// bm_trace_packet.h (wave packets); bm_trace.hip (the product kernels and their launchers),
// bm_rays.hip (ray queries) and bm_trace_ab.hip (trace variants measured slower and kept for A/B
// builds only, -DBM_TRACE_AB=1) each include what they launch. Everything here lives
// in an anonymous namespace: each translation unit instantiates the templates it launches.
//
// Semantics: closest hit with t > 0; equal t resolved to the lowest global triangle id (the order
// the reference's serial leaf lists give, BuildTree.cu:419-425); Möller-Trumbore and shading in
// the reference's operation order (CudaComon.cuh:117-155, 253-266). Bit-identical to
// oracle/beam_oracle.c orc_bvh_trace, including the node/triangle counters of the COUNT build.
#pragma once
#include <mutex>
#include <unordered_map>

#include "bm_internal.h"

namespace bm {
namespace {


// Blocks of one kernel the device keeps resident at once (its occupancy x CUs), cached per kernel.
template <typename K>
uint32_t resident_blocks(K kernel, uint32_t block) {
    static std::mutex mu;
    static std::unordered_map<const void*, uint32_t> cache;
    std::lock_guard<std::mutex> lock(mu);
    const void* key = reinterpret_cast<const void*>(kernel);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int dev = 0, per_cu = 0;
    hipDeviceProp_t prop;
    uint32_t n = 1024;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) == hipSuccess && per_cu > 0)
        n = (uint32_t)per_cu * (uint32_t)prop.multiProcessorCount;
    cache.emplace(key, n);
    return n;
}

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;

// Occupancy knob of the persistent trace kernels (A/B builds: -DBM_TRACE_WAVES_PER_EU=n asks the
// compiler to fit n waves per SIMD).
#ifndef BM_TRACE_WAVES_PER_EU
#define BM_TRACE_WAVES_PER_EU 0
#endif
#if BM_TRACE_WAVES_PER_EU > 0
#define BM_TRACE_OCCUPANCY __attribute__((amdgpu_waves_per_eu(BM_TRACE_WAVES_PER_EU)))
#else
#define BM_TRACE_OCCUPANCY
#endif

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum Ovf { OVF_NONE = 0, OVF_SCRATCH = 1, OVF_GLOBAL = 2 };

// Slab test of one child box, t = (box - o) * inv per plane (the reference's formulation,
// CudaComon.cuh:158-172; an FMA form box*inv - o*inv loses conservativeness for axis-parallel
// rays, inf - inf). A NaN plane (box plane through the eye, parallel ray) leaves that axis
// unconstrained; an all-NaN box never hits.
__device__ __forceinline__ bool child_hit(const float* lo, const float* hi, const vec3f o, const vec3f inv,
                                          float tbest, float& tn_out) {
    const float tlx = (lo[0] - o.x) * inv.x, thx = (hi[0] - o.x) * inv.x;
    const float tly = (lo[1] - o.y) * inv.y, thy = (hi[1] - o.y) * inv.y;
    const float tlz = (lo[2] - o.z) * inv.z, thz = (hi[2] - o.z) * inv.z;
    const float tn = fmaxf(fmaxf(fminf(tlx, thx), fminf(tly, thy)), fminf(tlz, thz));
    const float tf = fminf(fminf(fmaxf(tlx, thx), fmaxf(tly, thy)), fmaxf(tlz, thz));
    tn_out = tn;
    return (tn <= tf) && (tf >= 0.0f) && (tn <= tbest);
}

// A global load the compiler cannot merge with an LDS load (see QStack::get in bm_trace_quad.h); rare path: it waits
// for all of the wave's vector memory operations.
__device__ __forceinline__ uint32_t ovf_load(const uint32_t* ptr) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}

template <int LDS_N, int OVF>
struct Stack {
    uint32_t (*s_ref)[BLOCK];
    float (*s_t)[BLOCK];
    int tid;
    // overflow: global [depth][slot] (OVF_GLOBAL) or private (OVF_SCRATCH)
    uint32_t* g_ref;
    float* g_t;
    uint32_t stride;
    uint32_t x_ref[OVF == OVF_SCRATCH ? MAX_STACK - LDS_N : 1];
    float x_t[OVF == OVF_SCRATCH ? MAX_STACK - LDS_N : 1];

    __device__ __forceinline__ void put(int sp, uint32_t ref, float t) {
        if (OVF == OVF_NONE && sp >= LDS_N) return;  // experiment-only variant: drops (never faults)
        if (OVF == OVF_NONE || sp < LDS_N) {
            s_ref[sp][tid] = ref;
            s_t[sp][tid] = t;
        } else if (OVF == OVF_SCRATCH) {
            x_ref[sp - LDS_N] = ref;
            x_t[sp - LDS_N] = t;
        } else {
            g_ref[(size_t)(sp - LDS_N) * stride] = ref;
            g_t[(size_t)(sp - LDS_N) * stride] = t;
        }
    }
    __device__ __forceinline__ void get(int sp, uint32_t& ref, float& t) const {
        if (OVF == OVF_NONE && sp >= LDS_N) {
            ref = EMPTY_REF;
            t = __builtin_inff();
            return;
        }
        if (OVF == OVF_NONE || sp < LDS_N) {
            ref = s_ref[sp][tid];
            t = s_t[sp][tid];
        } else if (OVF == OVF_SCRATCH) {
            ref = x_ref[sp - LDS_N];
            t = x_t[sp - LDS_N];
        } else {
            ref = ovf_load(&g_ref[(size_t)(sp - LDS_N) * stride]);  // not mergeable into a flat load
            t = u2f(ovf_load(reinterpret_cast<const uint32_t*>(&g_t[(size_t)(sp - LDS_N) * stride])));
        }
    }
};

// orient * ray with a glm mat3 (column-major m[c*3+r]; type_mat3x3.inl:427-429 row sums).
__device__ __forceinline__ vec3f orient_mul(const float* m, const vec3f r) {
    return v3((m[0] * r.x + m[3] * r.y) + m[6] * r.z, (m[1] * r.x + m[4] * r.y) + m[7] * r.z,
              (m[2] * r.x + m[5] * r.y) + m[8] * r.z);
}

// Camera::setInitialRays (Camera.cpp:61-66) for pixel (x, gy), then dir = orient * ray.
__device__ __forceinline__ vec3f primary_dir(const TraceParams& p, uint32_t x, uint32_t gy) {
    const float rx = p.rx[x], ry = p.ry[gy];
    const float d = 1.f / sqrtf(p.z2 + rx * rx + ry * ry);
    return orient_mul(p.orient, v3(rx * d, ry * d, p.zoom * d));
}

// Raises the wave's issue priority once it has run `after` traversal steps (wave-uniform count).
// Waves still traversing then hold the frame's critical path (grazing silhouette rays).
// The level is fixed (2): levels 1-3 measured alike, and a runtime level costs a
// chain of scalar compares and branches in every traversal step.
template <uint32_t PRIO_AFTER>
__device__ __forceinline__ void prio_boost(const TraceParams& p, uint32_t& iter) {
    if (PRIO_AFTER) {
        iter = __builtin_amdgcn_readfirstlane(iter) + 1u;
        if (iter == p.prio_after) __builtin_amdgcn_s_setprio(2);
    }
}

// tri_test (Möller-Trumbore with the exact-safe early reject): bm_common.h

__device__ __forceinline__ uint32_t global_row(const TraceParams& p, uint32_t lr) {
    if (p.band_step == 1 && p.band_first == 0) return lr;  // whole frame: no integer division
    return ((lr / p.band_h) * p.band_step + p.band_first) * p.band_h + lr % p.band_h;
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(const TraceParams& p, unsigned long long n, unsigned long long t,
                                               unsigned long long h, const unsigned long long (&sh)[3]) {
    if (COUNT) {
        atomicAdd(&p.counters[0], n);
        atomicAdd(&p.counters[1], t);
        atomicAdd(&p.counters[2], h);
        if (p.shadow_counters)
            for (int k = 0; k < 3; ++k) atomicAdd(&p.shadow_counters[k], sh[k]);
    }
}

// Shadow modes of the primary kernels: none, fused (the pixel's own thread traces its shadow ray
// right after the primary hit, so shadow work interleaves with primary work over the whole
// persistent grid) or queue (hit pixels compacted for k_shadow_persistent, the wavefront form).
enum ShadowMode { SH_NONE = 0, SH_FUSED = 1, SH_QUEUE = 2 };

// Shadow segment of a primary hit at distance t: origin pulled back towards the eye by
// t * (1 - 1e-4), direction to the light (unnormalised).
__device__ __forceinline__ void shadow_segment(const TraceParams& p, const vec3f eye, const vec3f dir, float t,
                                               vec3f& o, vec3f& d) {
    const float ts = t * 0.9999f;
    o = v3(eye.x + dir.x * ts, eye.y + dir.y * ts, eye.z + dir.z * ts);
    d = v3(p.light[0] - o.x, p.light[1] - o.y, p.light[2] - o.z);
}

// bmFaceInterpolate<vec3> + normalize + pack (CudaComon.cuh:253-266, BuildTree.cu:489-491) of the
// corner normals n[9] at (bu, bv): the packed framebuffer entry of a hit (red = trunc(|n.z| * 255)),
// z = the normalised n.z.
__device__ __forceinline__ uint32_t shade_normals(const float* n, float bu, float bv, float& z) {
    const float ww = 1.f - (bu + bv);
    const vec3f nn = v3((n[0] * ww + n[3] * bu) + n[6] * bv, (n[1] * ww + n[4] * bu) + n[7] * bv,
                        (n[2] * ww + n[5] * bu) + n[8] * bv);
    const float il = 1.f / sqrtf(dot(nn, nn));
    z = nn.z * il;
    const float rr = fabsf(z * 255.f);
    return ((rr == rr) ? (uint32_t)rr : 0u) << 16;
}

// shade_normals of triangle id's normals; nzv receives |n.z|.
__device__ __forceinline__ uint32_t shade_hit(const TraceParams& p, uint32_t id, float bu, float bv, float& nzv) {
    float z;
    const uint32_t packed = shade_normals(p.nrm + 9 * (size_t)id, bu, bv, z);
    nzv = fabsf(z);
    return packed;
}

// DIAG (bm_camera_trace_profile, never timed): per wave, s_memrealtime (100 MHz) at start and end,
// (XCC id << 32 | HW_ID) and the sum over its tiles of the tile's longest per-lane work (node
// records + triangle tests; needs COUNT).
// Adds to diag_work the longest of the wave's lanes' work on one tile.
template <typename T>
__device__ __forceinline__ void diag_add_tile(T& diag_work, unsigned long long lane_work) {
    uint32_t wl = (uint32_t)lane_work;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wl = max(wl, (uint32_t)__shfl_xor((int)wl, o));
    diag_work += wl;
}

// Writes wave w's record at the end of its kernel.
__device__ __forceinline__ void diag_wave_record(const TraceParams& p, int w, int lane, uint64_t t_start,
                                                 uint64_t diag_work) {
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) {
        // HW_REG_HW_ID (id 4, all 32 bits) and HW_REG_XCC_ID (id 20, bits 3:0)
        const uint32_t hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
        const size_t wv = (size_t)blockIdx.x * WAVES + w;
        p.diag[4 * wv + 0] = t_start;
        p.diag[4 * wv + 1] = t_end;
        p.diag[4 * wv + 2] = ((uint64_t)xcc << 32) | hwid;
        p.diag[4 * wv + 3] = diag_work;
    }
}

// Persistent launch on min(p.persistent_blocks, the kernel's resident blocks); *grid gets the size.
template <typename K>
void launch_persistent(K kernel, const TraceParams& p, hipStream_t s, uint32_t* grid) {
    const uint32_t g = std::min(p.persistent_blocks, resident_blocks(kernel, BLOCK));
    if (grid) *grid = g;
    kernel<<<g, BLOCK, 0, s>>>(p);
}

}  // namespace
}  // namespace bm
