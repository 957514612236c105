// bm_sat_dev.h — the reference's triangle/box separating-axis test (triBoxOverlap, BoxTriangle.cuh:134-222)
// as the reference-mode kd build wrote it (bm_kd.hip) and as the box overlap query uses it (bm_boxes.hip):
// "this box holds this triangle" means the same to both. The text stands here as its first user wrote it.
#pragma once
#include "bm_internal.h"

namespace bm {
namespace {

// planeBoxOverlap (BoxTriangle.cuh:57-79)
__device__ __forceinline__ bool plane_box(const float* nrm, const float* vert, const float* maxbox) {
    float vmin[3], vmax[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float v = vert[q];
        if (nrm[q] > 0.0f) {
            vmin[q] = -maxbox[q] - v;
            vmax[q] = maxbox[q] - v;
        } else {
            vmin[q] = maxbox[q] - v;
            vmax[q] = -maxbox[q] - v;
        }
    }
    // (dot(vmin) > 0 -> false; dot(vmax) >= 0 -> true; else false), as one expression
    return !((nrm[0] * vmin[0] + nrm[1] * vmin[1]) + nrm[2] * vmin[2] > 0.0f) &&
           (nrm[0] * vmax[0] + nrm[1] * vmax[1]) + nrm[2] * vmax[2] >= 0.0f;
}

__device__ __forceinline__ bool axis_sep(float pa, float pb, float rad) {
    float mn, mx;
    if (pa < pb) {
        mn = pa;
        mx = pb;
    } else {
        mn = pb;
        mx = pa;
    }
    return (mn > rad || mx < -rad);
}

// triBoxOverlap (BoxTriangle.cuh:134-222): the nine cross-axis tests (AXISTEST_* order), the AABB
// test (FINDMINMAX) and the plane test, operation for operation (same operands, same order, no
// contraction) but without the reference's early returns: its function has no side effects, so "false
// at the first separating test, else the plane test" equals "no test separates, and the plane test
// passes". Straight-line code: a wave whose lanes separate at different tests does not run the union
// of the return paths with their exec-mask saves (the descent walks ran at ~5k cycles per level with
// the branches).
// The test groups of tri_box, each with the reference's operations.
struct SatFrame {
    float v0[3], v1[3], v2[3], e0[3], e1[3], e2[3];
};
__device__ __forceinline__ void sat_frame(const float* bc, const float* tv, SatFrame& f) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.v0[c] = tv[c] - bc[c];
        f.v1[c] = tv[3 + c] - bc[c];
        f.v2[c] = tv[6 + c] - bc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.e0[c] = f.v1[c] - f.v0[c];
        f.e1[c] = f.v2[c] - f.v1[c];
        f.e2[c] = f.v0[c] - f.v2[c];
    }
}
// edge e0's three cross-axis tests (AXISTEST_X01, _Y02, _Z12)
__device__ __forceinline__ bool sat_sep_e0(const SatFrame& f, const float* hs) {
    const float* v0 = f.v0; const float* v1 = f.v1; const float* v2 = f.v2; const float* e0 = f.e0;
    bool sep = false;
    float fx, fy, fz, a, b, pa, pb, rad;
    fx = fabsf(e0[0]); fy = fabsf(e0[1]); fz = fabsf(e0[2]);
    a = e0[2]; b = e0[1];
    pa = a * v0[1] - b * v0[2]; pb = a * v2[1] - b * v2[2];
    rad = fz * hs[1] + fy * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e0[2]; b = e0[0];
    pa = -a * v0[0] + b * v0[2]; pb = -a * v2[0] + b * v2[2];
    rad = fz * hs[0] + fx * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e0[1]; b = e0[0];
    pa = a * v1[0] - b * v1[1]; pb = a * v2[0] - b * v2[1];
    rad = fy * hs[0] + fx * hs[1];
    sep |= axis_sep(pb, pa, rad);
    return sep;
}
// edge e1's (AXISTEST_X01, _Y02, _Z0)
__device__ __forceinline__ bool sat_sep_e1(const SatFrame& f, const float* hs) {
    const float* v0 = f.v0; const float* v1 = f.v1; const float* v2 = f.v2; const float* e1 = f.e1;
    bool sep = false;
    float fx, fy, fz, a, b, pa, pb, rad;
    fx = fabsf(e1[0]); fy = fabsf(e1[1]); fz = fabsf(e1[2]);
    a = e1[2]; b = e1[1];
    pa = a * v0[1] - b * v0[2]; pb = a * v2[1] - b * v2[2];
    rad = fz * hs[1] + fy * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e1[2]; b = e1[0];
    pa = -a * v0[0] + b * v0[2]; pb = -a * v2[0] + b * v2[2];
    rad = fz * hs[0] + fx * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e1[1]; b = e1[0];
    pa = a * v0[0] - b * v0[1]; pb = a * v1[0] - b * v1[1];
    rad = fy * hs[0] + fx * hs[1];
    sep |= axis_sep(pa, pb, rad);
    return sep;
}
// edge e2's (AXISTEST_X2, _Y1, _Z12)
__device__ __forceinline__ bool sat_sep_e2(const SatFrame& f, const float* hs) {
    const float* v0 = f.v0; const float* v1 = f.v1; const float* v2 = f.v2; const float* e2 = f.e2;
    bool sep = false;
    float fx, fy, fz, a, b, pa, pb, rad;
    fx = fabsf(e2[0]); fy = fabsf(e2[1]); fz = fabsf(e2[2]);
    a = e2[2]; b = e2[1];
    pa = a * v0[1] - b * v0[2]; pb = a * v1[1] - b * v1[2];
    rad = fz * hs[1] + fy * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e2[2]; b = e2[0];
    pa = -a * v0[0] + b * v0[2]; pb = -a * v1[0] + b * v1[2];
    rad = fz * hs[0] + fx * hs[2];
    sep |= axis_sep(pa, pb, rad);
    a = e2[1]; b = e2[0];
    pa = a * v1[0] - b * v1[1]; pb = a * v2[0] - b * v2[1];
    rad = fy * hs[0] + fx * hs[1];
    sep |= axis_sep(pb, pa, rad);
    return sep;
}
// the AABB test (FINDMINMAX per axis)
__device__ __forceinline__ bool sat_sep_box(const SatFrame& f, const float* hs) {
    bool sep = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float mn = f.v0[c], mx = f.v0[c];
        if (f.v1[c] < mn) mn = f.v1[c];
        if (f.v1[c] > mx) mx = f.v1[c];
        if (f.v2[c] < mn) mn = f.v2[c];
        if (f.v2[c] > mx) mx = f.v2[c];
        sep |= (mn > hs[c] || mx < -hs[c]);
    }
    return sep;
}
__device__ __forceinline__ bool sat_plane(const SatFrame& f, const float* hs) {
    float nrm[3];
    nrm[0] = f.e0[1] * f.e1[2] - f.e0[2] * f.e1[1];
    nrm[1] = f.e0[2] * f.e1[0] - f.e0[0] * f.e1[2];
    nrm[2] = f.e0[0] * f.e1[1] - f.e0[1] * f.e1[0];
    return plane_box(nrm, f.v0, hs);
}
__device__ __forceinline__ bool tri_box(const float* bc, const float* hs, const float* tv) {
    SatFrame f;
    sat_frame(bc, tv, f);
    const bool sep = sat_sep_e0(f, hs) | sat_sep_e1(f, hs) | sat_sep_e2(f, hs) | sat_sep_box(f, hs);
    return !sep && sat_plane(f, hs);
}

}  // namespace
}  // namespace bm
