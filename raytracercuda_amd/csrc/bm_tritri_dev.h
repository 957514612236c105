// bm_tritri_dev.h — the triangle/triangle test of the triangle overlap query (bm_tris.hip), tri_tri of
// include/beam_c.h ("triangle overlap queries") statement for statement: an AABB part on the raw
// coordinates, comparisons only, and a seventeen-axis separating-axis part on coordinates translated by the
// query triangle's first vertex. float32, one rounding per operation in the order written (the library is
// built with -ffp-contract=off); a comparison with NaN is false. A conjunction without side effects and
// without early returns, for the reason bm_sat_dev.h gives: a wave whose lanes separate at different axes
// would otherwise run the union of the return paths.
#pragma once
#include "bm_internal.h"

namespace bm {
namespace {

// The query triangle as a quad keeps it between leaves: the translation, its own translated vertices
// (p0 = 0), its edges and normal, and its raw bounds, which are also the node test's.
struct TriQuery {
    float o[3];                    // a.v0
    float p1[3], p2[3];            // a.v1 - a.v0, a.v2 - a.v0
    float ea1[3], ea2[3];          // p2 - p1, 0 - p2 (eA0 is p1 - 0 = p1)
    float na[3];                   // eA0 x eA1
    float qlo[3], qhi[3];          // min and max of a's raw vertices
};

__device__ __forceinline__ float tt_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// the components as sat_plane writes them
__device__ __forceinline__ void tt_cross(const float* u, const float* v, float* d) {
    d[0] = u[1] * v[2] - u[2] * v[1];
    d[1] = u[2] * v[0] - u[0] * v[2];
    d[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ void tri_query(const float* a0, const float* a1, const float* a2, TriQuery& t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.o[k] = a0[k];
        t.p1[k] = a1[k] - a0[k];
        t.p2[k] = a2[k] - a0[k];
        float lo = a0[k], hi = a0[k];
        if (a1[k] < lo) lo = a1[k];
        if (a1[k] > hi) hi = a1[k];
        if (a2[k] < lo) lo = a2[k];
        if (a2[k] > hi) hi = a2[k];
        t.qlo[k] = lo;
        t.qhi[k] = hi;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t.ea1[k] = t.p2[k] - t.p1[k];
        t.ea2[k] = 0.0f - t.p2[k];
    }
    tt_cross(t.p1, t.ea1, t.na);
}

// axis d separates: A's interval over (0, d.p1, d.p2), B's over (d.q0, d.q1, d.q2)
__device__ __forceinline__ bool tt_sep(const float* d, const TriQuery& t, const float* q0, const float* q1,
                                       const float* q2) {
    const float a1 = tt_dot(d, t.p1), a2 = tt_dot(d, t.p2);
    const float b0 = tt_dot(d, q0), b1 = tt_dot(d, q1), b2 = tt_dot(d, q2);
    float mna = 0.0f, mxa = 0.0f;
    if (a1 < mna) mna = a1;
    if (a1 > mxa) mxa = a1;
    if (a2 < mna) mna = a2;
    if (a2 > mxa) mxa = a2;
    float mnb = b0, mxb = b0;
    if (b1 < mnb) mnb = b1;
    if (b1 > mxb) mxb = b1;
    if (b2 < mnb) mnb = b2;
    if (b2 > mxb) mxb = b2;
    return (mxa < mnb) | (mxb < mna);
}

// tri_tri(a, b): t holds a; b0, b1, b2 are the scene triangle's vertices as the build's record gives them
// (v0, v0 + e1, v0 + e2).
__device__ __forceinline__ bool tri_tri(const TriQuery& t, const float* b0, const float* b1, const float* b2) {
    bool apart = false;  // the AABB part, on the raw coordinates
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float lo = b0[k], hi = b0[k];
        if (b1[k] < lo) lo = b1[k];
        if (b1[k] > hi) hi = b1[k];
        if (b2[k] < lo) lo = b2[k];
        if (b2[k] > hi) hi = b2[k];
        apart |= !((lo <= t.qhi[k]) & (hi >= t.qlo[k]));
    }
    float q0[3], q1[3], q2[3], eb[3][3], nb[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q0[k] = b0[k] - t.o[k];
        q1[k] = b1[k] - t.o[k];
        q2[k] = b2[k] - t.o[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        eb[0][k] = q1[k] - q0[k];
        eb[1][k] = q2[k] - q1[k];
        eb[2][k] = q0[k] - q2[k];
    }
    tt_cross(eb[0], eb[1], nb);
    const float* ea[3] = {t.p1, t.ea1, t.ea2};
    bool sep = tt_sep(t.na, t, q0, q1, q2) | tt_sep(nb, t, q0, q1, q2);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            tt_cross(ea[i], eb[j], d);
            sep |= tt_sep(d, t, q0, q1, q2);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tt_cross(t.na, ea[i], d);
        sep |= tt_sep(d, t, q0, q1, q2);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        tt_cross(nb, eb[j], d);
        sep |= tt_sep(d, t, q0, q1, q2);
    }
    return !apart & !sep;
}

}  // namespace
}  // namespace bm
