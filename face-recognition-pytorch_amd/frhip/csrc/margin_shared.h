// What the fused head (head.hip) and the explicit-logit kernels (margin.hip) share so the two cannot drift apart: the margin constants,
// the validity tests of the margin descriptors (frhip_margin_t, frhip_margin_rows_t, frhip_margin_curr_t, frhip_margin_bce_t in
// frhip.h), the target element of the per-row margin, both elements of CurricularFace and both elements of the sigmoid (BCE) head.
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

// ---- the sigmoid (binary cross-entropy) head: UniFace / SphereFace2 (frhip_margin_bce_t in frhip.h)
// What the kernels take: ArcFace's constants of (s, m) for kind ARC (m3 = 0), or m3 = m for kind COS; the negatives' additive margin,
// the two weights and the device scalar b.
struct MarginBce : MarginConst { float m3, m_neg, w_pos, w_neg; int arc; const float* bias; };

// nullptr for a descriptor the kernels implement, else what is wrong with it (for frhip_last_error)
inline const char* margin_bce_desc_error(const frhip_margin_bce_t* mg) {
    if (!mg) return "null descriptor";
    if (!mg->bias) return "null bias";
    if (mg->kind != FRHIP_MARGIN_ARCFACE && mg->kind != FRHIP_MARGIN_COSFACE) return "kind is neither ARCFACE nor COSFACE";
    if (!(mg->s > 0.f) || !std::isfinite(mg->s)) return "s must be positive and finite";
    if (!std::isfinite(mg->m) || !std::isfinite(mg->m_neg)) return "m and m_neg must be finite";
    if (mg->kind == FRHIP_MARGIN_ARCFACE && !(mg->m >= 0.f && mg->m < 3.14159265358979f)) return "ARCFACE needs m in [0, pi)";
    if (!(mg->w_pos >= 0.f) || !(mg->w_neg >= 0.f) || !std::isfinite(mg->w_pos) || !std::isfinite(mg->w_neg))
        return "w_pos and w_neg must be finite and >= 0";
    if (mg->w_pos == 0.f && mg->w_neg == 0.f) return "w_pos and w_neg are both 0";
    return nullptr;
}

inline MarginBce margin_bce(const frhip_margin_bce_t* mg) {
    MarginBce mb;
    const bool arc = mg->kind == FRHIP_MARGIN_ARCFACE;
    static_cast<MarginConst&>(mb) = margin_const(mg->s, arc ? mg->m : 0.f);
    mb.m3 = arc ? 0.f : mg->m;
    mb.m_neg = mg->m_neg; mb.w_pos = mg->w_pos; mb.w_neg = mg->w_neg;
    mb.arc = arc ? 1 : 0;
    mb.bias = mg->bias;
    return mb;
}

// softplus(x) = log(1 + exp(x)) = max(x, 0) + log1p(exp(-|x|)): keeps its relative accuracy for x << 0, where log(1 + e) rounds to 0
// (at 122 000 classes nearly every negative term is that small)
__device__ __forceinline__ float bce_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// sigmoid(a) from e = exp(-|a|): 1 / (1 + e) for a >= 0, e / (1 + e) below -- no overflow, full relative accuracy in both tails
__device__ __forceinline__ float bce_sigmoid(float a) {
    const float e = expf(-fabsf(a));
    return (a >= 0.f ? 1.f : e) / (1.f + e);
}

// One element, on a cosine c already clamped to [-1, 1]; b = *mc.bias.  Both return the element's loss term and set a (the argument of
// the sigmoid), dcos = d term / d c (the caller zeroes it where the clamp of the raw cosine binds) and db = d term / d b.
// The target: a = s phi(c) - b, phi ArcFace's rule (curr_target, value and slope) or c - m; term w_pos softplus(-a).
__device__ __forceinline__ float bce_target(float c, const MarginBce& mc, float b, float& a, float& dcos, float& db) {
    float slope = 1.f, phi;
    if (mc.arc) phi = curr_target(c, mc, slope);
    else phi = c - mc.m3;
    a = fmaf(mc.s, phi, -b);
    const float sg = mc.w_pos * bce_sigmoid(-a);
    dcos = -sg * mc.s * slope;
    db = sg;
    return mc.w_pos * bce_softplus(-a);
}

// A non-target: a = s (c + m_neg) - b; term w_neg softplus(a).
__device__ __forceinline__ float bce_negative(float c, const MarginBce& mc, float b, float& a, float& dcos, float& db) {
    a = fmaf(mc.s, c + mc.m_neg, -b);
    const float sg = mc.w_neg * bce_sigmoid(a);
    dcos = sg * mc.s;
    db = -sg;
    return mc.w_neg * bce_softplus(a);
}

// bce.hip: rowloss[m] = sum_g part_loss[g][m], rowdb likewise, in float64 and in group order; launched by the head's forward entry points
int bce_rowfold_launch(const float* part_loss, const float* part_db, int groups, int n, float* rowloss, float* rowdb, hipStream_t stream,
                       const char* who);

}  // namespace frhip
