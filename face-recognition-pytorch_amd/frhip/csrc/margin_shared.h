// What the fused head (head.hip) and the explicit-logit kernels (margin.hip) share so the two cannot drift apart: the margin constants,
// the validity tests of the margin descriptors (frhip_margin_t, frhip_margin_rows_t, frhip_margin_curr_t in frhip.h), the target element
// of the per-row margin and both elements of CurricularFace.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "frhip.h"

namespace frhip {

// ArcFace(s, m): cos m, sin m, theta = cos(pi - m), sinmm = m sin(pi - m), rounded once from float64
struct MarginConst { float s, cos_m, sin_m, theta, sinmm; };

inline MarginConst margin_const(float s, float m) {
    MarginConst mc;
    const double pi = 3.14159265358979323846;
    mc.s = s; mc.cos_m = (float)cos((double)m); mc.sin_m = (float)sin((double)m);
    mc.theta = (float)cos(pi - (double)m); mc.sinmm = (float)(sin(pi - (double)m) * (double)m);
    return mc;
}

// a descriptor the kernels implement
inline bool margin_desc_ok(const frhip_margin_t* mg) {
    return mg && (mg->kind == FRHIP_MARGIN_ARCFACE || mg->kind == FRHIP_MARGIN_COSFACE) && mg->filter_thr >= 0.f;
}

inline bool margin_rows_desc_ok(const frhip_margin_rows_t* mg) {
    return mg && mg->m_ang && mg->m_add && mg->eps > 0.f && mg->eps < 0.5f;
}

// CurricularFace: both pointers set and the margin in [0, pi) (a NaN fails)
inline bool margin_curr_desc_ok(const frhip_margin_curr_t* mg) {
    return mg && mg->thr && mg->t && mg->m >= 0.f && mg->m < 3.14159265358979f;
}

// t: the target cosine, already clamped to [-1 + eps, 1 - eps].  Returns cos(clamp(theta + m_ang, eps, pi - eps)) - m_add and sets
// slope = d/dt = sin(theta + m_ang) / sin(theta), 0 where the clip of the angle binds.
// u = theta + m_ang only decides the branch; inside the clip cos(u) = t cos(m_ang) - sin(theta) sin(m_ang) and
// sin(u) / sin(theta) = cos(m_ang) + t sin(m_ang) / sin(theta): the ArcFace forms, nothing goes back through acos.
__device__ __forceinline__ float rows_margin_target(float t, float m_ang, float m_add, float eps, float& slope) {
    const float pi = 3.14159265358979f, u = acosf(t) + m_ang;
    if (u < eps || u > pi - eps) {
        slope = 0.f;
        return (u < eps ? cosf(eps) : -cosf(eps)) - m_add;
    }
    float sa, ca;
    sincosf(m_ang, &sa, &ca);
    const float sin_t = sqrtf((1.f - t) * (1.f + t));      // 1 - t is exact near t = 1 - eps, where 1 - t * t would lose five digits
    slope = ca + t * sa / sin_t;
    return t * ca - sin_t * sa - m_add;
}

// CurricularFace (frhip_margin_curr_t in frhip.h), on a cosine c already clamped to [-1, 1]; both return the value that is then x s and
// set slope = d/dc.
// The target: ArcFace's rule, cos(theta + m) above cos(pi - m), c - m sin(pi - m) below.
__device__ __forceinline__ float curr_target(float c, const MarginConst& mc, float& slope) {
    const float sin_t = sqrtf(1.f - c * c);
    if (c > mc.theta) { slope = mc.cos_m + c * mc.sin_m / sin_t; return c * mc.cos_m - sin_t * mc.sin_m; }
    slope = 1.f;
    return c - mc.sinmm;
}

// A non-target: hard where c > thr (strictly; thr = the row's cos(theta_y + m)), then c (tt + c) with tt the running mean of the target
// cosines; else c itself.  The sum is formed first and the product once: exact in fp32 whenever c (tt + c) is representable.
__device__ __forceinline__ float curr_negative(float c, float thr, float tt, float& slope) {
    if (c > thr) { slope = tt + 2.f * c; return c * (tt + c); }
    slope = 1.f;
    return c;
}

}  // namespace frhip
