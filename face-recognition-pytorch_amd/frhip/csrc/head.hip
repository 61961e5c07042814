// Fused margin-softmax head for gfx950 (PartialFC / ArcFace / distributed softmax cross-entropy).
//   forward : l2-normalise -> cos(theta) GEMM (MFMA) -> clamp -> additive angular margin on the target column ->
//             x s -> per-row online max / sum-exp partials.  Logits are never written to HBM.
//   backward: the same GEMM is recomputed, the tile is turned into d(loss)/d(cos) in registers and stored once
//             (compute dtype); dW = dT^T E and dE = dT W then run on the TN GEMM.
// Reference chain this replaces (file:line in /root/reference):
//   nets/PartialFC.py:198-204 normalize + linear + clamp, nets/ArcFace.py:76-91 margin,
//   nets/PartialFC.py:441-484 DistCrossEntropyFunc forward/backward.
// Cross-rank steps (all-reduce MAX / SUM of the per-row scalars) are done by the host between these kernels.
// The other margin modules of the reference (nets/ArcFace.py:5-61 CombinedMarginLoss with interclass filtering and easy_margin,
// :94-106 CosFace) are compile-time variants of the same epilogue (template arguments MK, FILT of head_epilogue), and so is the per-row
// margin (MG_ROWS: AdaFace and MagFace, not in the reference), whose two margins per row come from adaface_margins_kernel or
// magface_margins_kernel below; MagFace's gradient through the norms is magface_norm_grad_kernel and l2norm_bwd_norm*_kernel.
// CurricularFace (MG_CURR, not in the reference) is the one variant that also changes the non-target elements by a per-row test; its
// thresholds come from curricular_rows_kernel (curricular.hip).
// The sigmoid head (MG_BCE: UniFace / SphereFace2, not in the reference) is no softmax at all: head_epilogue_bce below; what follows its
// partials (row fold, rank pair, merge) is bce.hip.
#include <type_traits>
#include "igemm_nt.h"
#include "margin_shared.h"
#include "frhip.h"

namespace frhip {

struct MarginConstEx : MarginConst { float m3, thr; };       // CosFace margin, interclass-filtering threshold

// margin variants of the head epilogue.  The ArcFace kernel (the reference default, bench.py) keeps the plain MarginConst
// argument, so its kernel-argument layout and code are exactly those it had before the variants existed.
// (named constants and a traits struct, not an unnamed enum in std::conditional: the kernels' mangled names must come out the same in the
// host and the device compilation, and an unnamed type is numbered differently in the two)
constexpr int MG_ARC = 0, MG_ARC_EASY = 1, MG_COS = 2, MG_ROWS = 3, MG_CURR = 4, MG_BCE = 5;
struct MarginRows { float s, eps; const float* m_ang; const float* m_add; };      // per-row margins: [M] angular, [M] additive
struct MarginCurr : MarginConst { const float* thr; const float* t; };            // CurricularFace: [M] thresholds, the device scalar t
template <int MK, bool FILT> struct MarginArgOf { typedef MarginConstEx type; };
template <> struct MarginArgOf<MG_ARC, false> { typedef MarginConst type; };
template <> struct MarginArgOf<MG_ROWS, false> { typedef MarginRows type; };
template <> struct MarginArgOf<MG_CURR, false> { typedef MarginCurr type; };
template <> struct MarginArgOf<MG_BCE, false> { typedef MarginBce type; };                // margin_shared.h
template <int MK, bool FILT>
using MarginArg = typename MarginArgOf<MK, FILT>::type;

// one wave per row: xhat = x / max(|x|, eps) (T), norm (fp32)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, T* __restrict__ xhat,
                                                          float* __restrict__ norms, int rows, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float ss = 0.f;
    for (int j = lane * 4; j < D; j += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + j);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) ss += __shfl_xor(ss, d);
    const float nrm = fmaxf(sqrtf(ss), eps), inv = 1.f / nrm;
    if (lane == 0) norms[row] = nrm;
    T* o = xhat + (size_t)row * D;
    for (int j = lane * 4; j < D; j += 256) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[j + e] = from_f32<T>(v[e] * inv);
    }
}

// D == 512 (the embedding width of every configuration): a lane owns eight consecutive elements of its row -- 16-byte loads and stores,
// the row read ONCE and kept in registers, the row sum by DPP / permlane (no LDS permutes).  The generic kernels above / below issue
// 4- and 2-byte accesses and read the row twice (156 us for the 122 000 x 512 classifier in the backward pass).
__device__ __forceinline__ float wave_sum(float x) { return lane_sum_bit5(lane_sum_bit4(lane_sum_row16(x))); }

__global__ __launch_bounds__(256) void l2norm_rows512_kernel(const float* __restrict__ x, bf16_t* __restrict__ xhat,
                                                             float* __restrict__ norms, int rows, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * 512 + lane * 8;
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(xr), b = *reinterpret_cast<const f32x4_t*>(xr + 4);
    float ss = a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3] + b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3];
    ss = wave_sum(ss);
    const float nrm = fmaxf(sqrtf(ss), eps), inv = 1.f / nrm;
    if (lane == 0) norms[row] = nrm;
    bf16x8_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = (bf16_t)(a[e] * inv); o[4 + e] = (bf16_t)(b[e] * inv); }
    *reinterpret_cast<bf16x8_t*>(xhat + (size_t)row * 512 + lane * 8) = o;
}

__global__ __launch_bounds__(256) void l2norm_bwd512_kernel(const float* __restrict__ dxhat, const bf16_t* __restrict__ xhat,
                                                            const float* __restrict__ norms, float* __restrict__ dx, int rows,
                                                            float out_scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t off = (size_t)row * 512 + lane * 8;
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(dxhat + off), b = *reinterpret_cast<const f32x4_t*>(dxhat + off + 4);
    const bf16x8_t h = *reinterpret_cast<const bf16x8_t*>(xhat + off);
    float hv[8], dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) hv[e] = (float)h[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) dot += a[e] * hv[e] + b[e] * hv[4 + e];
    dot = wave_sum(dot);
    const float inv = out_scale / norms[row];
    f32x4_t oa, ob;
#pragma unroll
    for (int e = 0; e < 4; ++e) { oa[e] = (a[e] - hv[e] * dot) * inv; ob[e] = (b[e] - hv[4 + e] * dot) * inv; }
    *reinterpret_cast<f32x4_t*>(dx + off) = oa;
    *reinterpret_cast<f32x4_t*>(dx + off + 4) = ob;
}

// dx = (dxhat - xhat * <dxhat, xhat>) / norm     (all fp32 except xhat which is T)
template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ dxhat, const T* __restrict__ xhat,
                                                         const float* __restrict__ norms, float* __restrict__ dx,
                                                         int rows, int D, float out_scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* dr = dxhat + (size_t)row * D;
    const T* hr = xhat + (size_t)row * D;
    float dot = 0.f;
    for (int j = lane; j < D; j += 64) dot += dr[j] * to_f32<T>(hr[j]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) dot += __shfl_xor(dot, d);
    const float inv = out_scale / norms[row];
    for (int j = lane; j < D; j += 64) dx[(size_t)row * D + j] = (dr[j] - to_f32<T>(hr[j]) * dot) * inv;
}

// The two kernels above with the gradient of the norm itself folded in (frhip_l2norm_bwd_norm; MagFace, whose margin and regulariser
// depend on |x|): dx = ((dxhat - xhat <dxhat, xhat>) / norm + dnorm xhat) out_scale, d|x|/dx = xhat.  The tangential part goes through
// the same operations in the same order as above, so dnorm = 0 gives the bits of frhip_l2norm_bwd.
__global__ __launch_bounds__(256) void l2norm_bwd_norm512_kernel(const float* __restrict__ dxhat, const bf16_t* __restrict__ xhat,
                                                                 const float* __restrict__ norms, const float* __restrict__ dnorm,
                                                                 float* __restrict__ dx, int rows, float out_scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t off = (size_t)row * 512 + lane * 8;
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(dxhat + off), b = *reinterpret_cast<const f32x4_t*>(dxhat + off + 4);
    const bf16x8_t h = *reinterpret_cast<const bf16x8_t*>(xhat + off);
    float hv[8], dot = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) hv[e] = (float)h[e];
#pragma unroll
    for (int e = 0; e < 4; ++e) dot += a[e] * hv[e] + b[e] * hv[4 + e];
    dot = wave_sum(dot);
    const float inv = out_scale / norms[row], radial = dnorm[row] * out_scale;
    f32x4_t oa, ob;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        oa[e] = (a[e] - hv[e] * dot) * inv + hv[e] * radial;
        ob[e] = (b[e] - hv[4 + e] * dot) * inv + hv[4 + e] * radial;
    }
    *reinterpret_cast<f32x4_t*>(dx + off) = oa;
    *reinterpret_cast<f32x4_t*>(dx + off + 4) = ob;
}

template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_norm_kernel(const float* __restrict__ dxhat, const T* __restrict__ xhat,
                                                              const float* __restrict__ norms, const float* __restrict__ dnorm,
                                                              float* __restrict__ dx, int rows, int D, float out_scale) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* dr = dxhat + (size_t)row * D;
    const T* hr = xhat + (size_t)row * D;
    float dot = 0.f;
    for (int j = lane; j < D; j += 64) dot += dr[j] * to_f32<T>(hr[j]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) dot += __shfl_xor(dot, d);
    const float inv = out_scale / norms[row], radial = dnorm[row] * out_scale;
    for (int j = lane; j < D; j += 64) {
        const float h = to_f32<T>(hr[j]);
        dx[(size_t)row * D + j] = (dr[j] - h * dot) * inv + h * radial;
    }
}

// The epilogue of the sigmoid (BCE) head, same tile and arguments as head_epilogue below (which hands MG_BCE over to it): every element is
// a binary problem against the one threshold b = *mc.bias (read once per wave), rules bce_target / bce_negative of margin_shared.h.
// FWD = true : part_loss / part_db [group][m] = this 64-class column group's sums of the loss terms and of the d/db terms of row m;
//              ztarget[m] = a of the target; tsub as below.  Rows past M and classes past Nout add exactly 0: a padded column's cosine is
//              0, and unmasked it would add softplus(-b) to the loss.
// FWD = false: acc becomes d(loss)/d(cos) x gscale, from the element alone -- no row statistics are read; 0 where the clamp binds, in
//              rows past M and classes past Nout.
template <bool FWD, bool SUB>
__device__ __forceinline__ void head_epilogue_bce(int lane, const NtGeom& g, f32x4_t (&acc)[4][4], const uint32_t* win, int m0, int n0,
                                                  int group, const int* labels, const MarginBce& mc, float* part_loss, float* part_db,
                                                  float* ztarget, int* tsub, float gscale, const float* upstream) {
    const int fi = lane & 15, fg = lane >> 4;
    if (!FWD && upstream) gscale *= upstream[0];
    const float b = mc.bias[0];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int m = m0 + mt * 16 + fi;
        const bool mrow = m < g.M;
        const int lab = mrow ? labels[m] : -1;
        if constexpr (SUB)
            if (FWD && group == 0 && fg == 0 && mrow && lab < 0) tsub[m] = -1;
        float vl = 0.f, vd = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cls = n0 + nt * 16 + 4 * fg + e;
                const float raw = acc[nt][mt][e], c = fminf(fmaxf(raw, -1.f), 1.f);
                const bool tgt = cls == lab, live = cls < g.Nout && mrow;        // lab = -1 past M, and a label lies below Nout
                float a, dcos, db;
                const float term = tgt ? bce_target(c, mc, b, a, dcos, db) : bce_negative(c, mc, b, a, dcos, db);
                if (FWD) {
                    if (live) { vl += term; vd += db; }
                    if (tgt) {
                        ztarget[m] = a;
                        if constexpr (SUB) tsub[m] = (int)((win[nt] >> (2 * (4 * mt + e))) & 3u);
                    }
                } else {
                    acc[nt][mt][e] = (live && raw >= -1.f && raw <= 1.f) ? dcos * gscale : 0.f;
                }
            }
        if (FWD) {
            vl = lane_sum_bit5(lane_sum_bit4(vl));
            vd = lane_sum_bit5(lane_sum_bit4(vd));
            if (fg == 0 && mrow) {
                part_loss[(size_t)group * g.M + m] = vl;
                part_db[(size_t)group * g.M + m] = vd;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The epilogue of both head kernels, on one wave's 64 x 64 tile of cosines acc[nt][mt] (rows from m0, classes from n0).
// FWD = true : partial row max / sum-exp per 64-class column group, target logit.
// FWD = false: acc becomes d(loss)/d(cos), from the recomputed cosines and the global row max / sum; 0 in rows past M and classes past Nout.
// MK: MG_ARC (cos(theta + m), below cos(pi - m) t - m sin(pi - m)), MG_ARC_EASY (cos(theta + m) for t > 0, else t), MG_COS (t - m3),
// MG_ROWS (row m: every cosine clamped to [-1 + eps, 1 - eps], target cos(clamp(theta + m_ang[m], eps, pi - eps)) - m_add[m], slope 0 where
// a clamp binds; frhip_margin_rows_t in frhip.h), MG_CURR (the target as MG_ARC; a non-target of row m whose clamped cosine is > thr[m]
// becomes t (tt + t), slope tt + 2 t, tt = *mc.t read once per wave; a label -1 row has no exempt column; frhip_margin_curr_t in frhip.h),
// MG_BCE (no softmax: head_epilogue_bce above, with part_max / part_sum as its part_loss / part_db; rowmax / rowsum are not read).
// FILT: interclass filtering (reference nets/ArcFace.py:28-39): an element that is not its row's target and whose clamped cosine is
// > thr is multiplied by 0 -- logit 0, which still counts in the softmax sum, and d/dcos 0 (the reference builds the mask under
// no_grad); a row without a target on this shard (label -1) is filtered in every column.
// SUB (head_sub_kernel; win is not read otherwise): win[nt] holds the winning plane of element (mt, e) in bits 2 * (4 mt + e) .., and FWD
// writes tsub[m] = the winning plane of row m's target, -1 for a row whose label is -1.
// lane = lane_id(), from the kernel.  The margin goes by value and the pointers carry no __restrict__ (the kernels' own parameters do): with it
// the compiler emits other floating-point compares and selects in some instantiations than it did when this text stood in the kernels.
template <bool FWD, int MK, bool FILT, bool SUB>
__device__ __forceinline__ void head_epilogue(int lane, const NtGeom& g, f32x4_t (&acc)[4][4], const uint32_t* win, int m0, int n0,
                                              int group, const int* labels, MarginArg<MK, FILT> mc, float* part_max, float* part_sum,
                                              float* ztarget, int* tsub, const float* rowmax, const float* rowsum, float gscale,
                                              const float* upstream) {
    if constexpr (MK == MG_BCE) {
        head_epilogue_bce<FWD, SUB>(lane, g, acc, win, m0, n0, group, labels, mc, part_max, part_sum, ztarget, tsub, gscale, upstream);
        return;
    }
    const int fi = lane & 15, fg = lane >> 4;
    if (!FWD && upstream) gscale *= upstream[0];        // d(loss)/d(loss) stays on the device: no host sync
    [[maybe_unused]] float curr_t = 0.f, curr_thr = 2.f;                      // MG_CURR only
    if constexpr (MK == MG_CURR) curr_t = mc.t[0];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int m = m0 + mt * 16 + fi;
        const bool mrow = m < g.M;
        const int lab = mrow ? labels[m] : -1;
        float gm = 0.f, gs = 1.f;
        if (!FWD && mrow) { gm = rowmax[m]; gs = 1.f / rowsum[m]; }
        [[maybe_unused]] float tlo, thi, m_ang = 0.f, m_add = 0.f;            // MG_ROWS only: the other variants keep their literals
        if constexpr (MK == MG_ROWS) {
            tlo = -1.f + mc.eps; thi = 1.f - mc.eps;
            if (lab >= 0) { m_ang = mc.m_ang[m]; m_add = mc.m_add[m]; }       // lab >= 0 implies m < M
        }
        if constexpr (MK == MG_CURR) curr_thr = mrow ? mc.thr[m] : 2.f;       // every row of the batch has one, label -1 rows too
        if constexpr (SUB)
            if (FWD && group == 0 && fg == 0 && mrow && lab < 0) tsub[m] = -1;
        float z[4][4];
        float vmax = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cls = n0 + nt * 16 + 4 * fg + e;
                const float raw = acc[nt][mt][e];
                float t;
                if constexpr (MK == MG_ROWS) t = fminf(fmaxf(raw, tlo), thi);
                else t = fminf(fmaxf(raw, -1.f), 1.f);
                float slope = 1.f;
                bool filtered = false;
                if (cls == lab) {
                    if constexpr (MK == MG_ARC) {
                        const float sin_t = sqrtf(1.f - t * t);
                        if (t > mc.theta) { slope = mc.cos_m + t * mc.sin_m / sin_t; t = t * mc.cos_m - sin_t * mc.sin_m; }
                        else t = t - mc.sinmm;
                    } else if constexpr (MK == MG_ARC_EASY) {
                        const float sin_t = sqrtf(1.f - t * t);
                        if (t > 0.f) { slope = mc.cos_m + t * mc.sin_m / sin_t; t = t * mc.cos_m - sin_t * mc.sin_m; }
                    } else if constexpr (MK == MG_ROWS) {
                        t = rows_margin_target(t, m_ang, m_add, mc.eps, slope);
                    } else if constexpr (MK == MG_CURR) {
                        t = curr_target(t, mc, slope);
                    } else {
                        t = t - mc.m3;
                    }
                } else if constexpr (FILT) {
                    if (t > mc.thr) { t = 0.f; filtered = true; }
                } else if constexpr (MK == MG_CURR) {
                    t = curr_negative(t, curr_thr, curr_t, slope);
                }
                const float zz = t * mc.s;
                if (FWD) {
                    z[nt][e] = (cls < g.Nout) ? zz : -INFINITY;          // the padded classes of the last tile never enter a sum
                    vmax = fmaxf(vmax, z[nt][e]);
                    if (cls == lab && mrow) {
                        ztarget[m] = zz;
                        if constexpr (SUB) tsub[m] = (int)((win[nt] >> (2 * (4 * mt + e))) & 3u);
                    }
                } else {
                    float d = 0.f;
                    if (cls < g.Nout && mrow) {
                        const float p = __expf(zz - gm) * gs;
                        bool inside;
                        if constexpr (MK == MG_ROWS) inside = raw >= tlo && raw <= thi;
                        else inside = raw >= -1.f && raw <= 1.f && !filtered;
                        d = inside ? (p - (cls == lab ? 1.f : 0.f)) * gscale * mc.s * slope : 0.f;
                    }
                    acc[nt][mt][e] = d;
                }
            }
        if (FWD) {
            vmax = lane_max_bit5(lane_max_bit4(vmax));
            float vs = 0.f;
            const float vref = vmax == -INFINITY ? 0.f : vmax;                  // a fully masked group: sum 0, no NaN
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int e = 0; e < 4; ++e) vs += __expf(z[nt][e] - vref);      // exp(-inf) = 0 for masked classes
            vs = lane_sum_bit5(lane_sum_bit4(vs));
            if (fg == 0 && mrow) {
                part_max[(size_t)group * g.M + m] = vmax;
                part_sum[(size_t)group * g.M + m] = vs;
            }
        }
    }
}

// One wave's tile ml.acc through LDS to o[m][n] (row pitch ldt, columns below ncols) and, with ot set, transposed to ot[class][sample].
// stage_out begins with a barrier: whatever read the LDS before (the operand stages, the previous plane's tile) is done.
template <typename T>
__device__ __forceinline__ void head_store_tile(const NtGeom& g, NtMainloop<T, 2, 2>& ml, char* smem, int m0, int n0, T* o, int ldt,
                                                int ncols, T* ot, int ldtt) {
    constexpr int P = NtTile<T, 2, 2>::template stage_pitch<T>();
    constexpr int EPV = 16 / (int)sizeof(T), LPR = 64 / EPV, RPI = 64 / LPR;
    const char* mine = ml.template stage_out<T>(smem);
    const int lane = lane_id(), chunk = lane % LPR, rsub = lane / LPR;
    const int n = n0 + chunk * EPV;
    for (int it = 0; it < 64 / RPI; ++it) {
        const int row = it * RPI + rsub, m = m0 + row;
        if (m < g.M && n < ncols)         // columns in [Nout, ncols) hold zeros (dT pitch padding)
            *reinterpret_cast<Vec16<T>*>(o + (size_t)m * ldt + n) = *reinterpret_cast<const Vec16<T>*>(mine + row * P + chunk * 16);
    }
    if (ot) {
        // the same tile transposed, dTt[class][sample] (pitch ldtt, multiple of the 16-byte vector): the embedding-gradient GEMM
        // contracts over classes and wants class-major rows -- written here, a separate transpose pass (125 MB read + written at
        // 122 000 classes) is not needed.  Lane = class row of the tile, eight 16-byte vectors of samples each.
        const int cls = n0 + lane;
        if (cls < g.Nout) {
#pragma unroll
            for (int v = 0; v < 64 / EPV; ++v) {
                Vec16<T> tv;
#pragma unroll
                for (int e = 0; e < EPV; ++e) tv.v[e] = *reinterpret_cast<const T*>(mine + (v * EPV + e) * P + lane * (int)sizeof(T));
                const int mcol = m0 + v * EPV;
                if (mcol < ldtt) *reinterpret_cast<Vec16<T>*>(ot + (size_t)cls * ldtt + mcol) = tv;      // rows past M hold zeros (masked above)
            }
        }
    }
}

// One centre per class.  FWD: the forward partials; !FWD: the dT tile (compute dtype), and its transpose when dtt is set.
template <typename T, bool FWD, int MK, bool FILT>
__global__ __launch_bounds__(256, 2) void head_kernel(NtGeom g, const void* __restrict__ ehat,
                                                             const void* __restrict__ what, const int* __restrict__ labels,
                                                             MarginArg<MK, FILT> mc, float* __restrict__ part_max,
                                                             float* __restrict__ part_sum, float* __restrict__ ztarget,
                                                             const float* __restrict__ rowmax, const float* __restrict__ rowsum,
                                                             float gscale, const float* __restrict__ upstream,
                                                             void* __restrict__ dt, int ldt, void* __restrict__ dtt, int ldtt,
                                                             int mtiles, int ntiles) {
    typedef NtTile<T, 2, 2> Tile;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t lin = xcd_remap(blockIdx.x, gridDim.x);
    // mtile fastest: the (few) row tiles that share one weight tile run together on one XCD
    const int mtile = (int)(lin % (uint32_t)mtiles), ntile = (int)(lin / (uint32_t)mtiles);
    NtMainloop<T, 2, 2> ml;
    ml.run(g, ehat, what, smem, mtile, ntile, 0, g.ksteps);

    const int lane = lane_id(), wave = wave_id();
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = mtile * Tile::BM + wm * 64, n0 = ntile * Tile::BN + wn * 64;
    // ntile * 2 + wn: the 64-class column group id
    head_epilogue<FWD, MK, FILT, false>(lane, g, ml.acc, nullptr, m0, n0, ntile * 2 + wn, labels, mc, part_max, part_sum, ztarget, nullptr,
                                        rowmax, rowsum, gscale, upstream);
    if (!FWD) head_store_tile<T>(g, ml, smem, m0, n0, reinterpret_cast<T*>(dt), ldt, ldt, reinterpret_cast<T*>(dtt), ldtt);
}

// ---------------------------------------------------------------------------------------------------------
// Sub-centre variant (sub-center ArcFace, Deng et al., ECCV 2020): class c owns K centres, what[k * Nout + c] (plane-major: plane k is
// a contiguous [Nout][D] table), and its cosine is the maximum over them.  The main loop runs once per plane against the same embedding
// tile; a running element-wise maximum of the accumulators and the winning plane (2 bits per element, strict > when moving to a higher
// plane: an exact tie stays with the lowest) are kept in registers, and the pooled tile enters head_epilogue.  FWD and
// the recompute do the same arithmetic on the same operands in the same order, so they pick the same winner bit for bit.
//   FWD : additionally tsub[m] = winning plane of row m's target, -1 for a row whose label is -1.
//   !FWD: d = d loss / d cos_c from the pooled cosine, once; then K tiles, plane k holding d where it won and an exact 0 elsewhere:
//         dT[m][k * ldp + c] (ldp = the planes' column pitch, a whole number of 16-byte vectors; columns [Nout, ldp) of a plane zero),
//         dTt[k * Nout + c][m].
// A kernel of its own around the shared epilogue and tile store, not a switch inside head_kernel: the second accumulator tile and the
// winner bits cost registers (189 - 253 VGPRs against 114 - 120, half the waves per SIMD), and with one centre per class the library
// launches head_kernel with the arguments it always had.
constexpr int HEAD_SUB_MAX = 4;              // winners are packed 2 bits each: 16 elements of one nt column per 32-bit register

template <typename T, bool FWD, int MK, bool FILT>
__global__ __launch_bounds__(256, 2) void head_sub_kernel(NtGeom g, const void* __restrict__ ehat,
                                                                 const void* __restrict__ what, const int* __restrict__ labels,
                                                                 MarginArg<MK, FILT> mc, int K, float* __restrict__ part_max,
                                                                 float* __restrict__ part_sum, float* __restrict__ ztarget,
                                                                 int* __restrict__ tsub, const float* __restrict__ rowmax,
                                                                 const float* __restrict__ rowsum, float gscale,
                                                                 const float* __restrict__ upstream, void* __restrict__ dt, int ldt,
                                                                 int ldp, void* __restrict__ dtt, int ldtt, int mtiles, int ntiles) {
    typedef NtTile<T, 2, 2> Tile;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t lin = xcd_remap(blockIdx.x, gridDim.x);
    const int mtile = (int)(lin % (uint32_t)mtiles), ntile = (int)(lin / (uint32_t)mtiles);
    NtMainloop<T, 2, 2> ml;
    f32x4_t best[4][4];
    uint32_t win[4] = {0u, 0u, 0u, 0u};                  // win[nt]: plane of element (mt, e) in bits 2 * (4 mt + e) ..
    for (int k = 0; k < K; ++k) {
        if (k) __syncthreads();                         // every wave is done reading the previous plane's operand stages
        ml.run(g, ehat, reinterpret_cast<const char*>(what) + (size_t)k * g.b_bytes, smem, mtile, ntile, 0, g.ksteps);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = ml.acc[nt][mt][e];
                    if (k == 0) best[nt][mt][e] = v;
                    else if (v > best[nt][mt][e]) {
                        best[nt][mt][e] = v;
                        win[nt] = (win[nt] & ~(3u << (2 * (4 * mt + e)))) | ((uint32_t)k << (2 * (4 * mt + e)));
                    }
                }
    }

    const int lane = lane_id(), wave = wave_id();
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = mtile * Tile::BM + wm * 64, n0 = ntile * Tile::BN + wn * 64;
    head_epilogue<FWD, MK, FILT, true>(lane, g, best, win, m0, n0, ntile * 2 + wn, labels, mc, part_max, part_sum, ztarget, tsub, rowmax,
                                       rowsum, gscale, upstream);
    if (!FWD)
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        ml.acc[nt][mt][e] = ((win[nt] >> (2 * (4 * mt + e))) & 3u) == (uint32_t)k ? best[nt][mt][e] : 0.f;
            // plane k: columns [Nout, ldp) of the plane hold zeros
            head_store_tile<T>(g, ml, smem, m0, n0, reinterpret_cast<T*>(dt) + (size_t)k * ldp, ldt, ldp,
                               dtt ? reinterpret_cast<T*>(dtt) + (size_t)k * g.Nout * ldtt : nullptr, ldtt);
        }
}

// rowmax[m] = max_g part_max[g][m]; rowsum[m] = sum_g part_sum[g][m] * exp(part_max[g][m] - rowmax[m])
// block = 16 rows x 16 group-lanes; each lane folds its share of the column groups with an online max/sum merge,
// the 16 partial (max, sum) pairs of a row are merged through LDS.
__global__ __launch_bounds__(256) void head_rowreduce_kernel(const float* __restrict__ part_max, const float* __restrict__ part_sum,
                                                             int ngroups, int N, float* __restrict__ rowmax, float* __restrict__ rowsum) {
    __shared__ float smax[16][17], ssum[16][17];
    const int ml = threadIdx.x & 15, gl = threadIdx.x >> 4;
    const int m = blockIdx.x * 16 + ml;
    float mx = -INFINITY, s = 0.f;
    if (m < N) {
        for (int gq = gl; gq < ngroups; gq += 16) {
            const float pm = part_max[(size_t)gq * N + m], ps = part_sum[(size_t)gq * N + m];
            if (pm > mx) { s = s * __expf(mx - pm) + ps; mx = pm; }
            else if (pm > -INFINITY) s += ps * __expf(pm - mx);
        }
    }
    smax[gl][ml] = mx; ssum[gl][ml] = s;
    __syncthreads();
    if (gl == 0 && m < N) {
        float M = -INFINITY;
#pragma unroll
        for (int k = 0; k < 16; ++k) M = fmaxf(M, smax[k][ml]);
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) if (smax[k][ml] > -INFINITY) S += ssum[k][ml] * __expf(smax[k][ml] - M);
        rowmax[m] = M; rowsum[m] = S;
    }
}

// rowsum *= exp(local_max - global_max)      (before the cross-rank SUM)
__global__ void head_rescale_kernel(float* __restrict__ rowsum, const float* __restrict__ local_max,
                                    const float* __restrict__ global_max, int N) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < N) rowsum[m] *= __expf(local_max[m] - global_max[m]);
}

// q[m] = owned ? exp(z_target - M)/S : 0
__global__ void head_target_prob_kernel(const float* __restrict__ ztarget, const int* __restrict__ labels,
                                        const float* __restrict__ rowmax, const float* __restrict__ rowsum,
                                        float* __restrict__ q, int N) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < N) q[m] = labels[m] >= 0 ? __expf(ztarget[m] - rowmax[m]) / rowsum[m] : 0.f;
}

// Cross-shard merge of the per-row softmax statistics in ONE exchange (reference nets/PartialFC.py:448, :453, :459 issues an
// all-reduce MAX and two all-reduce SUMs).  Every rank packs {local max, local sum-exp, target logit or -inf} per row; the
// packed [N][3] blocks of all ranks are all-gathered and every rank folds them in rank order (same result on every rank).
__global__ void head_pack_stats_kernel(const float* __restrict__ ztarget, const int* __restrict__ labels,
                                       const float* __restrict__ rowmax, const float* __restrict__ rowsum,
                                       float* __restrict__ packed, int N) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < N) {
        packed[3 * m + 0] = rowmax[m];
        packed[3 * m + 1] = rowsum[m];
        packed[3 * m + 2] = labels[m] >= 0 ? ztarget[m] : -INFINITY;
    }
}

// gathered [ws][N][3] -> global max M, global sum S = sum_r s_r exp(m_r - M), q = exp(z_owner - M) / S (0: nobody owns the row)
__global__ void head_merge_stats_kernel(const float* __restrict__ gathered, int ws, int N, float* __restrict__ gmax,
                                        float* __restrict__ gsum, float* __restrict__ q) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= N) return;
    float M = -INFINITY;
    for (int r = 0; r < ws; ++r) M = fmaxf(M, gathered[((size_t)r * N + m) * 3]);
    float S = 0.f, num = 0.f;
    for (int r = 0; r < ws; ++r) {
        const float* g = gathered + ((size_t)r * N + m) * 3;
        S += g[1] * __expf(g[0] - M);
        if (g[2] > -INFINITY) num += __expf(g[2] - M);
    }
    gmax[m] = M; gsum[m] = S; q[m] = num / S;
}

// loss = -mean(log(max(q, 1e-30)))          single block
__global__ void head_loss_kernel(const float* __restrict__ q, int N, float* __restrict__ loss) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int m = threadIdx.x; m < N; m += 256) acc += logf(fmaxf(q[m], 1e-30f));
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = -red[0] / (float)N;
}

// the margin a launch runs with: the variant (mk, filt) and its kernel argument, ex for the descriptor variants, rows for MG_ROWS
struct HeadMargin { int mk; bool filt; MarginConstEx ex; MarginRows rows; MarginCurr curr; MarginBce bce; };

template <int MK, bool FILT>
static MarginArg<MK, FILT> margin_arg(const HeadMargin& hm) {
    if constexpr (MK == MG_ROWS) return hm.rows;
    else if constexpr (MK == MG_CURR) return hm.curr;
    else if constexpr (MK == MG_BCE) return hm.bce;
    else return hm.ex;                              // plain ArcFace: the MarginConst part only
}

// what the kernels take besides the geometry and the margin; a forward call leaves the backward's fields null and the other way round
struct HeadArgs {
    const void *ehat, *what;
    const int* labels;
    float *pmax, *psum, *zt;
    int* tsub;
    const float *rmax, *rsum;
    float gscale;
    const float* upstream;
    void* dt;
    int ldt, ldp;
    void* dtt;
    int ldtt;
};

// K = 0: head_kernel; K >= 1: head_sub_kernel over K planes
template <typename T, bool FWD, int MK, bool FILT>
static int head_launch_mk(const NtGeom& g, const HeadArgs& a, const HeadMargin& hm, int K, hipStream_t stream) {
    typedef NtTile<T, 2, 2> Tile;
    const int mtiles = (g.M + Tile::BM - 1) / Tile::BM, ntiles = (g.Nout + Tile::BN - 1) / Tile::BN;
    const int lds = Tile::template lds_bytes<T>();
    const MarginArg<MK, FILT> mc = margin_arg<MK, FILT>(hm);
    auto plain = head_kernel<T, FWD, MK, FILT>;
    auto sub = head_sub_kernel<T, FWD, MK, FILT>;
    const char* who = K ? "head_sub" : "head";
    if (set_dynamic_lds(K ? reinterpret_cast<const void*>(sub) : reinterpret_cast<const void*>(plain), lds, who)) return FRHIP_ELAUNCH;
    if (K)
        hipLaunchKernelGGL(sub, dim3(mtiles * ntiles), dim3(256), lds, stream, g, a.ehat, a.what, a.labels, mc, K, a.pmax, a.psum, a.zt,
                           a.tsub, a.rmax, a.rsum, a.gscale, a.upstream, a.dt, a.ldt, a.ldp, a.dtt, a.ldtt, mtiles, ntiles);
    else
        hipLaunchKernelGGL(plain, dim3(mtiles * ntiles), dim3(256), lds, stream, g, a.ehat, a.what, a.labels, mc, a.pmax, a.psum, a.zt,
                           a.rmax, a.rsum, a.gscale, a.upstream, a.dt, a.ldt, a.dtt, a.ldtt, mtiles, ntiles);
    return check_launch(who);
}

template <bool FWD>
static int head_launch(int dtype, const NtGeom& g, const HeadArgs& a, const HeadMargin& hm, int K, hipStream_t stream) {
#define HEAD_VARIANT(MKV, FV) \
    if (hm.mk == MKV && hm.filt == FV) \
        return dtype == FRHIP_DT_BF16 ? head_launch_mk<bf16_t, FWD, MKV, FV>(g, a, hm, K, stream) \
                                      : head_launch_mk<float, FWD, MKV, FV>(g, a, hm, K, stream);
    HEAD_VARIANT(MG_ARC, false)
    HEAD_VARIANT(MG_ARC, true)
    HEAD_VARIANT(MG_ARC_EASY, false)
    HEAD_VARIANT(MG_ARC_EASY, true)
    HEAD_VARIANT(MG_COS, false)
    HEAD_VARIANT(MG_COS, true)
    HEAD_VARIANT(MG_ROWS, false)
    HEAD_VARIANT(MG_CURR, false)
    HEAD_VARIANT(MG_BCE, false)
#undef HEAD_VARIANT
    set_error("head: unknown margin variant %d", hm.mk);
    return FRHIP_EINVAL;
}

// sub: the entry points that take K centres per class (`cl` is the number of classes; what holds K * cl rows, plane-major)
static int head_geom(NtGeom& g, int dtype, int n, int cl, int d, bool sub, int K, const char* who) {
    if (sub && (K < 1 || K > HEAD_SUB_MAX)) {
        set_error("%s: %d sub-centres per class (1 .. %d are supported)", who, K, HEAD_SUB_MAX);
        return FRHIP_EINVAL;
    }
    const int es = dtype == FRHIP_DT_BF16 ? 2 : 4, bke = NT_ROWB / es;
    if ((dtype != FRHIP_DT_BF16 && dtype != FRHIP_DT_F32) || n <= 0 || cl <= 0 || d <= 0 || (d % bke)) {
        set_error("%s: unsupported shape/dtype (n=%d classes=%d d=%d dtype=%d; d must be a multiple of %d)", who, n, cl, d, dtype, bke);
        return FRHIP_EINVAL;
    }
    if (1LL * cl * d * es > 0x7fffffffLL || 1LL * n * d * es > 0x7fffffffLL) { set_error("%s: operand exceeds 2 GiB", who); return FRHIP_EINVAL; }
    // the GEMMs behind the recompute kernel read all K planes as one table
    if (sub && 1LL * K * cl * d * es > 0x7fffffffLL) { set_error("%s: %d planes of %d classes exceed 2 GiB", who, K, cl); return FRHIP_EINVAL; }
    g.H = 1; g.W = 1; g.C = d; g.Ho = 1; g.Wo = 1; g.R = 1; g.S = 1; g.stride = 1; g.pad = 0; g.mode = 0;
    g.M = n; g.Nout = cl; g.Ktot = d; g.ksteps = d / bke; g.ksteps_per_split = g.ksteps;
    g.a_bytes = (uint32_t)(1LL * n * d * es); g.b_bytes = (uint32_t)(1LL * cl * d * es);
    g.par_a = -1; g.par_b = -1; g.hc = 0; g.wc = 0; g.par_r0 = 0; g.par_s0 = 0;
    return FRHIP_OK;
}

static int head_pitches(int dtype, int n, int cl, bool sub, int K, int ldt, int ldp, const void* dtt, int ldtt, const char* who) {
    const int epv = dtype == FRHIP_DT_BF16 ? 8 : 4;
    if (sub && (ldp < cl || (ldp % epv) || 1LL * ldt < 1LL * K * ldp || (ldt % epv))) {
        set_error("%s: bad dT pitches (row pitch %d, plane pitch %d, %d planes of %d classes)", who, ldt, ldp, K, cl);
        return FRHIP_EINVAL;
    }
    if (!sub && (ldt < cl || (ldt % epv))) { set_error("%s: bad dT pitch %d", who, ldt); return FRHIP_EINVAL; }
    if (dtt && (ldtt < n || (ldtt % epv))) { set_error("%s: bad transposed pitch %d", who, ldtt); return FRHIP_EINVAL; }
    return FRHIP_OK;
}

// descriptor -> (variant, constants); FRHIP_EINVAL for a descriptor the kernels do not implement
static int margin_desc(const frhip_margin_t* mg, HeadMargin& hm, const char* who) {
    if (!margin_desc_ok(mg)) {
        set_error("%s: bad margin descriptor (kind=%d thr=%g)", who, mg ? mg->kind : -1, mg ? (double)mg->filter_thr : 0.0);
        return FRHIP_EINVAL;
    }
    const bool arc = mg->kind == FRHIP_MARGIN_ARCFACE;
    static_cast<MarginConst&>(hm.ex) = margin_const(mg->s, arc ? mg->m : 0.f);
    hm.ex.m3 = arc ? 0.f : mg->m;
    hm.ex.thr = mg->filter_thr;
    hm.mk = arc ? (mg->easy ? MG_ARC_EASY : MG_ARC) : MG_COS;
    hm.filt = mg->filter_thr > 0.f;
    return FRHIP_OK;
}

static int margin_desc(const frhip_margin_rows_t* mg, HeadMargin& hm, const char* who) {
    if (!margin_rows_desc_ok(mg)) {
        set_error("%s: bad per-row margin descriptor (null pointer, or eps outside (0, 0.5))", who);
        return FRHIP_EINVAL;
    }
    hm.rows.s = mg->s; hm.rows.eps = mg->eps; hm.rows.m_ang = mg->m_ang; hm.rows.m_add = mg->m_add;
    hm.mk = MG_ROWS;
    hm.filt = false;
    return FRHIP_OK;
}

static int margin_desc(const frhip_margin_curr_t* mg, HeadMargin& hm, const char* who) {
    if (!margin_curr_desc_ok(mg)) {
        set_error("%s: bad CurricularFace descriptor (null descriptor, null thr or t, or m outside [0, pi))", who);
        return FRHIP_EINVAL;
    }
    static_cast<MarginConst&>(hm.curr) = margin_const(mg->s, mg->m);
    hm.curr.thr = mg->thr; hm.curr.t = mg->t;
    hm.mk = MG_CURR;
    hm.filt = false;
    return FRHIP_OK;
}

static int margin_desc(const frhip_margin_bce_t* mg, HeadMargin& hm, const char* who) {
    if (const char* why = margin_bce_desc_error(mg)) { set_error("%s: bad BCE descriptor: %s", who, why); return FRHIP_EINVAL; }
    hm.bce = margin_bce(mg);
    hm.mk = MG_BCE;
    hm.filt = false;
    return FRHIP_OK;
}

// The forward / recompute entry points.  D: frhip_margin_t, frhip_margin_rows_t, frhip_margin_curr_t or frhip_margin_bce_t (whose
// forward folds its partials with bce.hip's row fold instead of the max / sum-exp merge, and whose recompute gets no row statistics).  sub = false: head_kernel (K is not read);
// sub = true: head_sub_kernel over K planes, K = 1 included.  Every argument is validated before anything is launched.
template <typename D>
static int head_fwd_impl(const char* who, int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                         bool sub, int K, const D* margin, float* part_max, float* part_sum, float* ztarget, int* tsub, float* rowmax,
                         float* rowsum, hipStream_t stream) {
    NtGeom g;
    HeadMargin hm = {};
    int rc = by_dtype(dtype, who, [](auto) { return FRHIP_OK; });
    if (rc || (rc = head_geom(g, dtype, n, classes, d, sub, K, who)) || (rc = margin_desc(margin, hm, who))) return rc;
    HeadArgs a = {};
    a.ehat = ehat; a.what = what; a.labels = labels; a.pmax = part_max; a.psum = part_sum; a.zt = ztarget; a.tsub = tsub;
    if ((rc = head_launch<true>(dtype, g, a, hm, sub ? K : 0, stream))) return rc;
    if constexpr (std::is_same<D, frhip_margin_bce_t>::value)
        return bce_rowfold_launch(part_max, part_sum, frhip_head_groups(classes), n, rowmax, rowsum, stream, who);
    hipLaunchKernelGGL(head_rowreduce_kernel, dim3((n + 15) / 16), dim3(256), 0, stream, part_max, part_sum,
                       frhip_head_groups(classes), n, rowmax, rowsum);
    char tag[64];
    snprintf(tag, sizeof(tag), "%s/rowreduce", who);
    return check_launch(tag);
}

template <typename D>
static int head_bwd_dt_impl(const char* who, int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                            bool sub, int K, const D* margin, const float* rowmax, const float* rowsum, float gscale,
                            const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt, hipStream_t stream) {
    NtGeom g;
    HeadMargin hm = {};
    int rc = by_dtype(dtype, who, [](auto) { return FRHIP_OK; });
    if (rc || (rc = head_geom(g, dtype, n, classes, d, sub, K, who)) ||
        (rc = head_pitches(dtype, n, classes, sub, K, ldt, ldp, dtt, ldtt, who)) || (rc = margin_desc(margin, hm, who))) return rc;
    HeadArgs a = {};
    a.ehat = ehat; a.what = what; a.labels = labels; a.rmax = rowmax; a.rsum = rowsum; a.gscale = gscale; a.upstream = upstream;
    a.dt = dt; a.ldt = ldt; a.ldp = ldp; a.dtt = dtt; a.ldtt = ldtt;
    return head_launch<false>(dtype, g, a, hm, sub ? K : 0, stream);
}

// AdaFace's per-row margins from the embedding norms of the global batch (frhip_adaface_margins in frhip.h).  ONE block: n is a batch
// size, a few thousand floats; the mean and then the squared deviations from it are summed in float64.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    __syncthreads();                                    // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
    return r;
}

__device__ __forceinline__ double safe_norm(float x) { return (double)fminf(fmaxf(x, 0.001f), 100.f); }

__global__ __launch_bounds__(1024) void adaface_margins_kernel(const float* __restrict__ norms, int n, double m, double h, double t_alpha,
                                                               double eps, int update, float* __restrict__ batch_mean,
                                                               float* __restrict__ batch_std, float* __restrict__ m_ang,
                                                               float* __restrict__ m_add) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += safe_norm(norms[i]);
    const double mean = block_sum_f64(acc, red) / (double)n;
    acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double dv = safe_norm(norms[i]) - mean;
        acc += dv * dv;
    }
    const double sd = sqrt(block_sum_f64(acc, red) / (double)(n - 1));
    double bm = (double)batch_mean[0], bs = (double)batch_std[0];        // every thread reads the old values ...
    if (update) { bm = t_alpha * mean + (1.0 - t_alpha) * bm; bs = t_alpha * sd + (1.0 - t_alpha) * bs; }
    __syncthreads();                                                     // ... before thread 0 overwrites them
    if (update && threadIdx.x == 0) { batch_mean[0] = (float)bm; batch_std[0] = (float)bs; }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double k = fmin(fmax(h * (safe_norm(norms[i]) - bm) / (bs + eps), -1.0), 1.0);
        m_ang[i] = (float)(-m * k);
        m_add[i] = (float)(m + m * k);
    }
}

// Guard band of frhip_magface_norm_grad's test for "the clip of u bound": where it did, the forward kernel stored s cosf(eps) or its
// negative, and the cosine read back as z / s is within one ulp (6e-8) of that; two ulps of 1 cover it.  Rows whose u lies within
// ~0.22 eps inside the clip are taken for clipped as well (sin(u) ~ eps there: the term dropped is that small).
constexpr float MAGFACE_CLIP_BAND = 2.4e-7f;

// MagFace's per-row margins and its regulariser from the embedding norms of the global batch (frhip_magface_margins in frhip.h).  ONE
// block like the kernel above; reg is summed in float64 in an order that depends on n alone, so every rank gets the same bits from the
// same gathered norms.
__global__ __launch_bounds__(1024) void magface_margins_kernel(const float* __restrict__ norms, int n, double l_a, double u_a, double l_m,
                                                               double u_m, float* __restrict__ m_ang, float* __restrict__ m_add,
                                                               float* __restrict__ reg) {
    __shared__ double red[16];
    const double slope = (u_m - l_m) / (u_a - l_a), inv_ua2 = 1.0 / (u_a * u_a);
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = fmin(fmax((double)norms[i], l_a), u_a);
        m_ang[i] = (float)(l_m + slope * (a - l_a));
        m_add[i] = 0.f;
        acc += a * inv_ua2 + 1.0 / a;
    }
    const double sum = block_sum_f64(acc, red);
    if (threadIdx.x == 0) reg[0] = (float)(sum / (double)n);
}

// d loss / d norm of every row of the global batch (frhip_magface_norm_grad in frhip.h), from what the forward pass left per row: the
// owner's target logit (the entry above -inf among the ranks' packed blocks) gives cos(u), the global row max / sum-exp give q.
__global__ __launch_bounds__(256) void magface_norm_grad_kernel(const float* __restrict__ norms, const float* __restrict__ packed, int ws,
                                                                int n, const float* __restrict__ rowmax, const float* __restrict__ rowsum,
                                                                float s, float eps, double l_a, double u_a, double l_m, double u_m,
                                                                double lambda_g, double gscale, const float* __restrict__ upstream,
                                                                double out_scale, float* __restrict__ dnorm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = (double)norms[i];
    if (!(a > l_a && a < u_a)) { dnorm[i] = 0.f; return; }            // the clamp of the norm binds: margin and regulariser are constants
    float zt = -INFINITY;
    for (int r = 0; r < ws; ++r) zt = fmaxf(zt, packed[((size_t)r * n + i) * 3 + 2]);
    double dce = 0.0;
    if (zt > -INFINITY) {
        const float cu = zt / s;                                      // m_add = 0: the target logit is s cos(clamp(u))
        if (fabsf(cu) < cosf(eps) - MAGFACE_CLIP_BAND) {              // else the clip of u bound (or may have): no gradient to the margin
            const double q = exp((double)zt - (double)rowmax[i]) / (double)rowsum[i];
            dce = (double)s * sqrt((1.0 - (double)cu) * (1.0 + (double)cu)) * (1.0 - q) * gscale;
        }
    }
    const double g = dce * (u_m - l_m) / (u_a - l_a) + lambda_g * gscale * (1.0 / (u_a * u_a) - 1.0 / (a * a));
    dnorm[i] = (float)(g * (upstream ? (double)upstream[0] : 1.0) * out_scale);
}

}  // namespace frhip

using namespace frhip;

extern "C" int frhip_adaface_margins(const float* norms, int n, double m, double h, double t_alpha, double eps, int update,
                                     float* batch_mean, float* batch_std, float* m_ang, float* m_add, hipStream_t stream) {
    if (n < 2 || !norms || !batch_mean || !batch_std || !m_ang || !m_add) {
        set_error("frhip_adaface_margins: needs n >= 2 norms (n=%d) and non-null norms, batch_mean, batch_std, m_ang, m_add", n);
        return FRHIP_EINVAL;
    }
    hipLaunchKernelGGL(adaface_margins_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, norms, n, m, h, t_alpha, eps, update,
                       batch_mean, batch_std, m_ang, m_add);
    return check_launch("frhip_adaface_margins");
}

// the argument checks the two MagFace entry points share; `all_ptrs`: every pointer the entry point requires is non-null
static int magface_args(const char* who, int n, bool all_ptrs, const char* ptr_names, double l_a, double u_a) {
    if (n < 1 || !all_ptrs || !(u_a > l_a) || !(l_a > 0.0)) {
        set_error("%s: needs n >= 1 rows (n=%d), non-null %s, and 0 < l_a < u_a (l_a=%g u_a=%g)", who, n, ptr_names, l_a, u_a);
        return FRHIP_EINVAL;
    }
    return FRHIP_OK;
}

extern "C" int frhip_magface_margins(const float* norms, int n, double l_a, double u_a, double l_m, double u_m, float* m_ang,
                                     float* m_add, float* reg, hipStream_t stream) {
    if (const int rc = magface_args("frhip_magface_margins", n, norms && m_ang && m_add && reg, "norms, m_ang, m_add, reg", l_a, u_a)) return rc;
    hipLaunchKernelGGL(magface_margins_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, norms, n, l_a, u_a, l_m, u_m, m_ang, m_add,
                       reg);
    return check_launch("frhip_magface_margins");
}

extern "C" int frhip_magface_norm_grad(const float* norms, const float* packed, int world_size, int n, const float* rowmax,
                                       const float* rowsum, float s, float eps, double l_a, double u_a, double l_m, double u_m,
                                       double lambda_g, double gscale, const float* upstream, double out_scale, float* dnorm,
                                       hipStream_t stream) {
    if (const int rc = magface_args("frhip_magface_norm_grad", n, norms && packed && rowmax && rowsum && dnorm,
                                    "norms, packed, rowmax, rowsum, dnorm", l_a, u_a)) return rc;
    if (world_size < 1 || !(s > 0.f) || !(eps > 0.f && eps < 0.5f)) {
        set_error("frhip_magface_norm_grad: needs world_size >= 1, s > 0 and 0 < eps < 0.5 (ws=%d s=%g eps=%g)", world_size, s, eps);
        return FRHIP_EINVAL;
    }
    hipLaunchKernelGGL(magface_norm_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, norms, packed, world_size, n, rowmax, rowsum,
                       s, eps, l_a, u_a, l_m, u_m, lambda_g, gscale, upstream, out_scale, dnorm);
    return check_launch("frhip_magface_norm_grad");
}

extern "C" int frhip_head_sub_max(void) { return HEAD_SUB_MAX; }

extern "C" int frhip_head_groups(int num_classes) { return ((num_classes + 127) / 128) * 2; }

// ---- forward: one centre per class (head_kernel) ...
extern "C" int frhip_head_fwd_ex(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                 int d, const frhip_margin_t* margin, float* part_max, float* part_sum, float* ztarget,
                                 float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_ex", dtype, ehat, what, labels, n, classes, d, false, 1, margin, part_max, part_sum, ztarget, nullptr,
                         rowmax, rowsum, stream);
}

extern "C" int frhip_head_fwd(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                              int d, float s, float m, float* part_max, float* part_sum, float* ztarget,
                              float* rowmax, float* rowsum, hipStream_t stream) {
    const frhip_margin_t mg = {FRHIP_MARGIN_ARCFACE, 0, s, m, 0.f};
    return head_fwd_impl("frhip_head_fwd", dtype, ehat, what, labels, n, classes, d, false, 1, &mg, part_max, part_sum, ztarget, nullptr,
                         rowmax, rowsum, stream);
}

extern "C" int frhip_head_fwd_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                   int d, const frhip_margin_rows_t* margin, float* part_max, float* part_sum, float* ztarget,
                                   float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_rows", dtype, ehat, what, labels, n, classes, d, false, 1, margin, part_max, part_sum, ztarget,
                         nullptr, rowmax, rowsum, stream);
}

// ... and K sub-centres per class (head_sub_kernel).  `classes` is the number of classes; what holds K * classes rows, plane-major.
extern "C" int frhip_head_fwd_sub(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                  int subcenters, const frhip_margin_t* margin, float* part_max, float* part_sum, float* ztarget,
                                  int* tsub, float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_sub", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, part_max, part_sum,
                         ztarget, tsub, rowmax, rowsum, stream);
}

extern "C" int frhip_head_fwd_sub_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                       int subcenters, const frhip_margin_rows_t* margin, float* part_max, float* part_sum,
                                       float* ztarget, int* tsub, float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_sub_rows", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, part_max,
                         part_sum, ztarget, tsub, rowmax, rowsum, stream);
}

// ---- recompute (dT and its transpose), the same five
extern "C" int frhip_head_bwd_dt_ex(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                    int d, const frhip_margin_t* margin, const float* rowmax, const float* rowsum, float gscale,
                                    const float* upstream, void* dt, int ldt, void* dtt, int ldtt, hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_ex", dtype, ehat, what, labels, n, classes, d, false, 1, margin, rowmax, rowsum, gscale,
                            upstream, dt, ldt, 0, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                 int d, float s, float m, const float* rowmax, const float* rowsum, float gscale,
                                 const float* upstream, void* dt, int ldt, void* dtt, int ldtt, hipStream_t stream) {
    const frhip_margin_t mg = {FRHIP_MARGIN_ARCFACE, 0, s, m, 0.f};
    return head_bwd_dt_impl("frhip_head_bwd_dt", dtype, ehat, what, labels, n, classes, d, false, 1, &mg, rowmax, rowsum, gscale,
                            upstream, dt, ldt, 0, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                      int d, const frhip_margin_rows_t* margin, const float* rowmax, const float* rowsum, float gscale,
                                      const float* upstream, void* dt, int ldt, void* dtt, int ldtt, hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_rows", dtype, ehat, what, labels, n, classes, d, false, 1, margin, rowmax, rowsum, gscale,
                            upstream, dt, ldt, 0, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt_sub(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                     int subcenters, const frhip_margin_t* margin, const float* rowmax, const float* rowsum,
                                     float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                                     hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_sub", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, rowmax, rowsum,
                            gscale, upstream, dt, ldt, ldp, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt_sub_rows(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                          int subcenters, const frhip_margin_rows_t* margin, const float* rowmax, const float* rowsum,
                                          float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                                          hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_sub_rows", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, rowmax,
                            rowsum, gscale, upstream, dt, ldt, ldp, dtt, ldtt, stream);
}

// ---- CurricularFace: the four of the per-row margins with its descriptor
extern "C" int frhip_head_fwd_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                   int d, const frhip_margin_curr_t* margin, float* part_max, float* part_sum, float* ztarget,
                                   float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_curr", dtype, ehat, what, labels, n, classes, d, false, 1, margin, part_max, part_sum, ztarget,
                         nullptr, rowmax, rowsum, stream);
}

extern "C" int frhip_head_fwd_sub_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                       int subcenters, const frhip_margin_curr_t* margin, float* part_max, float* part_sum,
                                       float* ztarget, int* tsub, float* rowmax, float* rowsum, hipStream_t stream) {
    return head_fwd_impl("frhip_head_fwd_sub_curr", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, part_max,
                         part_sum, ztarget, tsub, rowmax, rowsum, stream);
}

extern "C" int frhip_head_bwd_dt_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes,
                                      int d, const frhip_margin_curr_t* margin, const float* rowmax, const float* rowsum, float gscale,
                                      const float* upstream, void* dt, int ldt, void* dtt, int ldtt, hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_curr", dtype, ehat, what, labels, n, classes, d, false, 1, margin, rowmax, rowsum, gscale,
                            upstream, dt, ldt, 0, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt_sub_curr(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                          int subcenters, const frhip_margin_curr_t* margin, const float* rowmax, const float* rowsum,
                                          float gscale, const float* upstream, void* dt, int ldt, int ldp, void* dtt, int ldtt,
                                          hipStream_t stream) {
    return head_bwd_dt_impl("frhip_head_bwd_dt_sub_curr", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, rowmax,
                            rowsum, gscale, upstream, dt, ldt, ldp, dtt, ldtt, stream);
}

// ---- the sigmoid (BCE) head: the four with its descriptor; null operands are refused here, everything else by the shared checks
static int bce_ptrs(const char* who, int dtype, bool ok) {
    if (const int rc = by_dtype(dtype, who, [](auto) { return FRHIP_OK; })) return rc;       // an unknown dtype is refused first, everywhere
    if (!ok) { set_error("%s: null pointer among the operands", who); return FRHIP_EINVAL; }
    return FRHIP_OK;
}

extern "C" int frhip_head_fwd_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                  const frhip_margin_bce_t* margin, float* part_loss, float* part_db, float* ztarget, float* rowloss,
                                  float* rowdb, hipStream_t stream) {
    if (const int rc = bce_ptrs("frhip_head_fwd_bce", dtype, ehat && what && labels && part_loss && part_db && ztarget && rowloss && rowdb)) return rc;
    return head_fwd_impl("frhip_head_fwd_bce", dtype, ehat, what, labels, n, classes, d, false, 1, margin, part_loss, part_db, ztarget,
                         nullptr, rowloss, rowdb, stream);
}

extern "C" int frhip_head_fwd_sub_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                      int subcenters, const frhip_margin_bce_t* margin, float* part_loss, float* part_db, float* ztarget,
                                      int* tsub, float* rowloss, float* rowdb, hipStream_t stream) {
    if (const int rc = bce_ptrs("frhip_head_fwd_sub_bce", dtype,
                                ehat && what && labels && part_loss && part_db && ztarget && tsub && rowloss && rowdb)) return rc;
    return head_fwd_impl("frhip_head_fwd_sub_bce", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, part_loss, part_db,
                         ztarget, tsub, rowloss, rowdb, stream);
}

extern "C" int frhip_head_bwd_dt_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                     const frhip_margin_bce_t* margin, float gscale, const float* upstream, void* dt, int ldt, void* dtt,
                                     int ldtt, hipStream_t stream) {
    if (const int rc = bce_ptrs("frhip_head_bwd_dt_bce", dtype, ehat && what && labels && dt)) return rc;
    return head_bwd_dt_impl("frhip_head_bwd_dt_bce", dtype, ehat, what, labels, n, classes, d, false, 1, margin, nullptr, nullptr, gscale,
                            upstream, dt, ldt, 0, dtt, ldtt, stream);
}

extern "C" int frhip_head_bwd_dt_sub_bce(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                         int subcenters, const frhip_margin_bce_t* margin, float gscale, const float* upstream, void* dt,
                                         int ldt, int ldp, void* dtt, int ldtt, hipStream_t stream) {
    if (const int rc = bce_ptrs("frhip_head_bwd_dt_sub_bce", dtype, ehat && what && labels && dt)) return rc;
    return head_bwd_dt_impl("frhip_head_bwd_dt_sub_bce", dtype, ehat, what, labels, n, classes, d, true, subcenters, margin, nullptr,
                            nullptr, gscale, upstream, dt, ldt, ldp, dtt, ldtt, stream);
}

extern "C" int frhip_l2norm_rows(int dtype, const float* x, void* xhat, float* norms, int rows, int d, float eps,
                                 hipStream_t stream) {
    return by_dtype(dtype, "frhip_l2norm_rows", [&](auto t) {
        typedef decltype(t) T;
        if (d % 4) { set_error("frhip_l2norm_rows: d must be a multiple of 4"); return FRHIP_EINVAL; }
        if (dtype == FRHIP_DT_BF16 && d == 512) hipLaunchKernelGGL(l2norm_rows512_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, (bf16_t*)xhat, norms, rows, eps);
        else hipLaunchKernelGGL(l2norm_rows_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, (T*)xhat, norms, rows, d, eps);
        return check_launch("frhip_l2norm_rows");
    });
}

extern "C" int frhip_l2norm_bwd(int dtype, const float* dxhat, const void* xhat, const float* norms, float* dx,
                                int rows, int d, float out_scale, hipStream_t stream) {
    return by_dtype(dtype, "frhip_l2norm_bwd", [&](auto t) {
        typedef decltype(t) T;
        if (dtype == FRHIP_DT_BF16 && d == 512) hipLaunchKernelGGL(l2norm_bwd512_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, dxhat, (const bf16_t*)xhat, norms, dx, rows, out_scale);
        else hipLaunchKernelGGL(l2norm_bwd_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, stream, dxhat, (const T*)xhat, norms, dx, rows, d, out_scale);
        return check_launch("frhip_l2norm_bwd");
    });
}

extern "C" int frhip_l2norm_bwd_norm(int dtype, const float* dxhat, const void* xhat, const float* norms, const float* dnorm, float* dx,
                                     int rows, int d, float out_scale, hipStream_t stream) {
    return by_dtype(dtype, "frhip_l2norm_bwd_norm", [&](auto t) {
        typedef decltype(t) T;
        if (rows < 1 || d < 1 || !dxhat || !xhat || !norms || !dnorm || !dx) {
            set_error("frhip_l2norm_bwd_norm: needs rows >= 1, d >= 1 (rows=%d d=%d) and non-null dxhat, xhat, norms, dnorm, dx", rows, d);
            return FRHIP_EINVAL;
        }
        if (dtype == FRHIP_DT_BF16 && d == 512) hipLaunchKernelGGL(l2norm_bwd_norm512_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, dxhat, (const bf16_t*)xhat, norms, dnorm, dx, rows, out_scale);
        else hipLaunchKernelGGL(l2norm_bwd_norm_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, stream, dxhat, (const T*)xhat, norms, dnorm, dx, rows, d, out_scale);
        return check_launch("frhip_l2norm_bwd_norm");
    });
}

extern "C" int frhip_head_rescale(float* rowsum, const float* local_max, const float* global_max, int n, hipStream_t stream) {
    hipLaunchKernelGGL(head_rescale_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rowsum, local_max, global_max, n);
    return check_launch("frhip_head_rescale");
}

extern "C" int frhip_head_target_prob(const float* ztarget, const int* labels, const float* rowmax, const float* rowsum,
                                      float* q, int n, hipStream_t stream) {
    hipLaunchKernelGGL(head_target_prob_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ztarget, labels, rowmax, rowsum, q, n);
    return check_launch("frhip_head_target_prob");
}

extern "C" int frhip_head_pack_stats(const float* ztarget, const int* labels, const float* rowmax, const float* rowsum,
                                     float* packed, int n, hipStream_t stream) {
    hipLaunchKernelGGL(head_pack_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, ztarget, labels, rowmax, rowsum, packed, n);
    return check_launch("frhip_head_pack_stats");
}

extern "C" int frhip_head_merge_stats(const float* gathered, int world_size, int n, float* rowmax, float* rowsum, float* q,
                                      hipStream_t stream) {
    if (world_size <= 0 || n <= 0) { set_error("frhip_head_merge_stats: bad shape (ws=%d n=%d)", world_size, n); return FRHIP_EINVAL; }
    hipLaunchKernelGGL(head_merge_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, gathered, world_size, n, rowmax, rowsum, q);
    return check_launch("frhip_head_merge_stats");
}

extern "C" int frhip_head_loss(const float* q, int n, float* loss, hipStream_t stream) {
    hipLaunchKernelGGL(head_loss_kernel, dim3(1), dim3(256), 0, stream, q, n, loss);
    return check_launch("frhip_head_loss");
}
