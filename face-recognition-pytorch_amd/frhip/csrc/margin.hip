// Explicit-logit versions of the margin and the class-sharded softmax cross-entropy, for callers that use the
// reference modules stand-alone (nets/ArcFace.py:76-105 ArcFace/CosFace.forward, nets/PartialFC.py:441-484
// DistCrossEntropyFunc).  The fused head (head.hip) never materialises logits; these kernels exist so that the
// drop-in nets.ArcFace / nets.PartialFC.DistCrossEntropy keep the reference's tensor-in / tensor-out contract.
// HBM-bound row kernels: one 256-thread block per row, 16-byte accesses where the row pitch allows.
#include "common.h"
#include "cross_pair.h"
#include "margin_shared.h"
#include "frhip.h"

namespace frhip {

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const float o = __shfl_xor(v, d); v = is_max ? fmaxf(v, o) : v + o; }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// out = s * margin(logits): kind 0 = ArcFace (cos(theta+m), fallback t - m sin(pi-m) below cos(pi-m); easy: cos(theta+m) for
// t > 0, else t), 1 = CosFace (t - m).  thr > 0: interclass filtering -- a non-target element > thr becomes 0 and its bit is set
// in filt (one 64-bit word per 64 columns, written by lane 0 of the wave that covers them).
// tsave[row] keeps the raw target cosine for the backward slope.  In place on `logits`.
__global__ __launch_bounds__(256) void margin_fwd_kernel(float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                         int C, float s, float cos_m, float sin_m, float theta,
                                                         float sinmm, float m3, int kind, float* __restrict__ tsave,
                                                         int easy, float thr, uint64_t* __restrict__ filt) {
    const int row = blockIdx.x;
    float* x = logits + (size_t)row * C;
    const int64_t lab = labels[row];
    const int words = (C + 63) / 64;
    for (int j = threadIdx.x; j < C; j += 256) {
        float t = x[j];
        bool dirty = false;
        if (j == lab) {
            tsave[row] = t;
            if (kind == 0) {
                const float sin_t = sqrtf(1.f - t * t);
                if (easy) t = t > 0.f ? t * cos_m - sin_t * sin_m : t;
                else t = t > theta ? t * cos_m - sin_t * sin_m : t - sinmm;
            } else {
                t = t - m3;
            }
        } else if (thr > 0.f && t > thr) {
            t = 0.f;
            dirty = true;
        }
        x[j] = t * s;
        if (filt) {
            const uint64_t bits = __ballot(dirty);
            if ((threadIdx.x & 63) == 0) filt[(size_t)row * words + j / 64] = bits;
        }
    }
}

__global__ __launch_bounds__(256) void margin_bwd_kernel(const float* __restrict__ gout, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ tsave, int C, float s, float cos_m,
                                                         float sin_m, float theta, int kind, float* __restrict__ gin,
                                                         int easy, const uint64_t* __restrict__ filt) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    const int words = (C + 63) / 64;
    for (int j = threadIdx.x; j < C; j += 256) {
        float gg = gout[(size_t)row * C + j] * s;
        if (j == lab && kind == 0) {
            const float t = tsave[row];
            if (t > (easy ? 0.f : theta)) gg *= cos_m + t * sin_m / sqrtf(1.f - t * t);
        }
        if (filt && ((filt[(size_t)row * words + j / 64] >> (j & 63)) & 1)) gg = 0.f;
        gin[(size_t)row * C + j] = gg;
    }
}

// Per-row margins (frhip_margin_rows_t, AdaFace) on explicit logits.  NOT in place: every element is clamped to [-1 + eps, 1 - eps] and
// the gradient is 0 where the clamp binds, which the backward decides from the caller's untouched input.
__global__ __launch_bounds__(256) void margin_fwd_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              int C, float s, float eps, const float* __restrict__ m_ang,
                                                              const float* __restrict__ m_add, float* __restrict__ out) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    for (int j = threadIdx.x; j < C; j += 256) {
        float t = fminf(fmaxf(logits[(size_t)row * C + j], -1.f + eps), 1.f - eps), slope;
        if (j == lab) t = rows_margin_target(t, m_ang[row], m_add[row], eps, slope);
        out[(size_t)row * C + j] = t * s;
    }
}

__global__ __launch_bounds__(256) void margin_bwd_rows_kernel(const float* __restrict__ gout, const float* __restrict__ logits,
                                                              const int64_t* __restrict__ labels, int C, float s, float eps,
                                                              const float* __restrict__ m_ang, const float* __restrict__ m_add,
                                                              float* __restrict__ gin) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    for (int j = threadIdx.x; j < C; j += 256) {
        const float raw = logits[(size_t)row * C + j];
        float gg = (raw >= -1.f + eps && raw <= 1.f - eps) ? gout[(size_t)row * C + j] * s : 0.f;
        if (j == lab) {
            float slope;
            rows_margin_target(fminf(fmaxf(raw, -1.f + eps), 1.f - eps), m_ang[row], m_add[row], eps, slope);
            gg *= slope;
        }
        gin[(size_t)row * C + j] = gg;
    }
}

// CurricularFace (frhip_margin_curr_t) on explicit logits: the element rules of the head's MG_CURR variant (margin_shared.h).  NOT in
// place: the backward rebuilds the clamp and the hard mask from the caller's untouched cosines.
__global__ __launch_bounds__(256) void margin_fwd_curr_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                              int C, MarginConst mc, const float* __restrict__ thr,
                                                              const float* __restrict__ tptr, float* __restrict__ out) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    const float row_thr = thr[row], tt = tptr[0];
    for (int j = threadIdx.x; j < C; j += 256) {
        float t = fminf(fmaxf(logits[(size_t)row * C + j], -1.f), 1.f), slope;
        t = j == lab ? curr_target(t, mc, slope) : curr_negative(t, row_thr, tt, slope);
        out[(size_t)row * C + j] = t * mc.s;
    }
}

__global__ __launch_bounds__(256) void margin_bwd_curr_kernel(const float* __restrict__ gout, const float* __restrict__ logits,
                                                              const int64_t* __restrict__ labels, int C, MarginConst mc,
                                                              const float* __restrict__ thr, const float* __restrict__ tptr,
                                                              float* __restrict__ gin) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    const float row_thr = thr[row], tt = tptr[0];
    for (int j = threadIdx.x; j < C; j += 256) {
        const float raw = logits[(size_t)row * C + j], t = fminf(fmaxf(raw, -1.f), 1.f);
        float slope;
        if (j == lab) curr_target(t, mc, slope);
        else curr_negative(t, row_thr, tt, slope);
        gin[(size_t)row * C + j] = (raw >= -1.f && raw <= 1.f) ? gout[(size_t)row * C + j] * mc.s * slope : 0.f;
    }
}

__global__ __launch_bounds__(256) void rows_max_kernel(const float* __restrict__ x, int C, float* __restrict__ rowmax) {
    __shared__ float red[4];
    const float* r = x + (size_t)blockIdx.x * C;
    float m = -INFINITY;
    for (int j = threadIdx.x; j < C; j += 256) m = fmaxf(m, r[j]);
    m = block_reduce(m, true, red);
    if (threadIdx.x == 0) rowmax[blockIdx.x] = m;
}

// x <- exp(x - rowmax) in place, rowsum = sum
__global__ __launch_bounds__(256) void rows_exp_sum_kernel(float* __restrict__ x, int C, const float* __restrict__ rowmax,
                                                           float* __restrict__ rowsum) {
    __shared__ float red[4];
    float* r = x + (size_t)blockIdx.x * C;
    const float m = rowmax[blockIdx.x];
    float s = 0.f;
    for (int j = threadIdx.x; j < C; j += 256) { const float e = __expf(r[j] - m); r[j] = e; s += e; }
    s = block_reduce(s, false, red);
    if (threadIdx.x == 0) rowsum[blockIdx.x] = s;
}

// x <- x / rowsum (probabilities); ptarget[row] = p at the label (0 when the label is -1)
__global__ __launch_bounds__(256) void rows_normalize_kernel(float* __restrict__ x, int C, const float* __restrict__ rowsum,
                                                             const int64_t* __restrict__ labels, float* __restrict__ ptarget) {
    float* r = x + (size_t)blockIdx.x * C;
    const float inv = 1.f / rowsum[blockIdx.x];
    const int64_t lab = labels[blockIdx.x];
    if (threadIdx.x == 0 && lab < 0) ptarget[blockIdx.x] = 0.f;
    for (int j = threadIdx.x; j < C; j += 256) {
        const float p = r[j] * inv;
        r[j] = p;
        if (j == lab) ptarget[blockIdx.x] = p;
    }
}

// grad = (p - onehot) / N * upstream   (in place on p)
__global__ __launch_bounds__(256) void ce_grad_kernel(float* __restrict__ p, int C, const int64_t* __restrict__ labels,
                                                      float inv_n, const float* __restrict__ upstream) {
    float* r = p + (size_t)blockIdx.x * C;
    const int64_t lab = labels[blockIdx.x];
    const float g = inv_n * upstream[0];
    for (int j = threadIdx.x; j < C; j += 256) r[j] = (r[j] - (j == lab ? 1.f : 0.f)) * g;
}

}  // namespace frhip

using namespace frhip;

extern "C" int frhip_margin_fwd_ex(float* logits, const int64_t* labels, int n, int c, const frhip_margin_t* margin, float* tsave,
                                   uint64_t* filtered, hipStream_t stream) {
    if (!margin_desc_ok(margin) || (margin->filter_thr > 0.f && !filtered)) {
        set_error("frhip_margin_fwd: bad margin descriptor or missing filter mask");
        return FRHIP_EINVAL;
    }
    if (n <= 0) return FRHIP_OK;
    const MarginConst mc = margin_const(margin->s, margin->m);
    hipLaunchKernelGGL(margin_fwd_kernel, dim3(n), dim3(256), 0, stream, logits, labels, c, mc.s, mc.cos_m, mc.sin_m, mc.theta, mc.sinmm,
                       margin->m, margin->kind, tsave, margin->easy, margin->filter_thr, margin->filter_thr > 0.f ? filtered : nullptr);
    return check_launch("frhip_margin_fwd");
}

extern "C" int frhip_margin_bwd_ex(const float* gout, const int64_t* labels, const float* tsave, const uint64_t* filtered, int n, int c,
                                   const frhip_margin_t* margin, float* gin, hipStream_t stream) {
    if (!margin_desc_ok(margin) || (margin->filter_thr > 0.f && !filtered)) {
        set_error("frhip_margin_bwd: bad margin descriptor or missing filter mask");
        return FRHIP_EINVAL;
    }
    if (n <= 0) return FRHIP_OK;
    const MarginConst mc = margin_const(margin->s, margin->m);
    hipLaunchKernelGGL(margin_bwd_kernel, dim3(n), dim3(256), 0, stream, gout, labels, tsave, c, mc.s, mc.cos_m, mc.sin_m, mc.theta,
                       margin->kind, gin, margin->easy, margin->filter_thr > 0.f ? filtered : nullptr);
    return check_launch("frhip_margin_bwd");
}

extern "C" int frhip_margin_fwd(float* logits, const int64_t* labels, int n, int c, float s, float m, int kind,
                                float* tsave, hipStream_t stream) {
    const frhip_margin_t mg = {kind, 0, s, m, 0.f};
    return frhip_margin_fwd_ex(logits, labels, n, c, &mg, tsave, nullptr, stream);
}

extern "C" int frhip_margin_bwd(const float* gout, const int64_t* labels, const float* tsave, int n, int c, float s,
                                float m, int kind, float* gin, hipStream_t stream) {
    const frhip_margin_t mg = {kind, 0, s, m, 0.f};
    return frhip_margin_bwd_ex(gout, labels, tsave, nullptr, n, c, &mg, gin, stream);
}

static int margin_rows_args(const frhip_margin_rows_t* mg, const void* a, const void* b, const void* c, const void* d, const char* who) {
    if (!margin_rows_desc_ok(mg) || !a || !b || !c || !d) {
        set_error("%s: null pointer, or eps outside (0, 0.5)", who);
        return FRHIP_EINVAL;
    }
    return FRHIP_OK;
}

extern "C" int frhip_margin_fwd_rows(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_rows_t* margin,
                                     float* out, hipStream_t stream) {
    if (n <= 0) return FRHIP_OK;
    if (margin_rows_args(margin, logits, labels, out, out, "frhip_margin_fwd_rows")) return FRHIP_EINVAL;
    hipLaunchKernelGGL(margin_fwd_rows_kernel, dim3(n), dim3(256), 0, stream, logits, labels, c, margin->s, margin->eps, margin->m_ang,
                       margin->m_add, out);
    return check_launch("frhip_margin_fwd_rows");
}

extern "C" int frhip_margin_bwd_rows(const float* gout, const float* logits, const int64_t* labels, int n, int c,
                                     const frhip_margin_rows_t* margin, float* gin, hipStream_t stream) {
    if (n <= 0) return FRHIP_OK;
    if (margin_rows_args(margin, gout, logits, labels, gin, "frhip_margin_bwd_rows")) return FRHIP_EINVAL;
    hipLaunchKernelGGL(margin_bwd_rows_kernel, dim3(n), dim3(256), 0, stream, gout, logits, labels, c, margin->s, margin->eps,
                       margin->m_ang, margin->m_add, gin);
    return check_launch("frhip_margin_bwd_rows");
}

static int margin_curr_args(const frhip_margin_curr_t* mg, const void* a, const void* b, const void* c, const void* d, const char* who) {
    if (!margin_curr_desc_ok(mg) || !a || !b || !c || !d) {
        set_error("%s: null pointer (an operand, the descriptor, its thr or t), or m outside [0, pi)", who);
        return FRHIP_EINVAL;
    }
    return FRHIP_OK;
}

extern "C" int frhip_margin_fwd_curr(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_curr_t* margin,
                                     float* out, hipStream_t stream) {
    if (margin_curr_args(margin, logits, labels, out, out, "frhip_margin_fwd_curr")) return FRHIP_EINVAL;
    if (n <= 0) return FRHIP_OK;
    hipLaunchKernelGGL(margin_fwd_curr_kernel, dim3(n), dim3(256), 0, stream, logits, labels, c, margin_const(margin->s, margin->m),
                       margin->thr, margin->t, out);
    return check_launch("frhip_margin_fwd_curr");
}

extern "C" int frhip_margin_bwd_curr(const float* gout, const float* logits, const int64_t* labels, int n, int c,
                                     const frhip_margin_curr_t* margin, float* gin, hipStream_t stream) {
    if (margin_curr_args(margin, gout, logits, labels, gin, "frhip_margin_bwd_curr")) return FRHIP_EINVAL;
    if (n <= 0) return FRHIP_OK;
    hipLaunchKernelGGL(margin_bwd_curr_kernel, dim3(n), dim3(256), 0, stream, gout, logits, labels, c, margin_const(margin->s, margin->m),
                       margin->thr, margin->t, gin);
    return check_launch("frhip_margin_bwd_curr");
}

extern "C" int frhip_rows_max(const float* x, int n, int c, float* rowmax, hipStream_t stream) {
    hipLaunchKernelGGL(rows_max_kernel, dim3(n), dim3(256), 0, stream, x, c, rowmax);
    return check_launch("frhip_rows_max");
}

extern "C" int frhip_rows_exp_sum(float* x, int n, int c, const float* rowmax, float* rowsum, hipStream_t stream) {
    hipLaunchKernelGGL(rows_exp_sum_kernel, dim3(n), dim3(256), 0, stream, x, c, rowmax, rowsum);
    return check_launch("frhip_rows_exp_sum");
}

extern "C" int frhip_rows_normalize(float* x, int n, int c, const float* rowsum, const int64_t* labels, float* ptarget,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(rows_normalize_kernel, dim3(n), dim3(256), 0, stream, x, c, rowsum, labels, ptarget);
    return check_launch("frhip_rows_normalize");
}

extern "C" int frhip_ce_grad(float* p, int n, int c, const int64_t* labels, float inv_n, const float* upstream,
                             hipStream_t stream) {
    hipLaunchKernelGGL(ce_grad_kernel, dim3(n), dim3(256), 0, stream, p, c, labels, inv_n, upstream);
    return check_launch("frhip_ce_grad");
}

// ---- verification pair scores (/root/reference/utils/eval.py:68-99): score = 1 - |a-b|^2 / 4 accumulated in float64
// from float32 differences in index order (the reference's arithmetic, so hist_idx = int(99999*score) is
// bit-exact), plus the two 100001-bin histograms by integer atomics.  One thread per pair.
namespace frhip {
__global__ void pair_score_kernel(const float* __restrict__ e1, const float* __restrict__ e2, const int64_t* __restrict__ labels,
                                  int n, int d, double* __restrict__ scores, int* __restrict__ hist_idx,
                                  int* __restrict__ hist_genuine, int* __restrict__ hist_imposter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int k = 0; k < d; ++k) {
        const float df = e1[(size_t)i * d + k] - e2[(size_t)i * d + k];
        const double dd = (double)df;
        sum += dd * dd;
    }
    const double score = 1.0 - sum / 4.0;
    const int idx = (int)((1e5 - 1.0) * score);
    scores[i] = score;
    hist_idx[i] = idx;
    if (idx >= 0 && idx <= 100000) atomicAdd(labels[i] ? hist_genuine + idx : hist_imposter + idx, 1);
}

// ---- cross-matching per-pair arithmetic: cross_acc / cross_pair_score (cross_pair.h) are shared by cross_score_kernel (pair
// list), cross_hist_kernel (histograms only) and the 1:N search (gallery_topk.hip) so the routes cannot drift apart.
// the reference's bin int(99999 * score); counted only when it lands in [0, 100000]
__device__ __forceinline__ int cross_bin(double score) { return (int)((1e5 - 1.0) * score); }
// threshold slot: the smallest t in [0, 100001] with score <= t / 1e5, where t / 1e5 is the correctly rounded double quotient that
// Python's `th / 1e5` computes (scores <= 0 go to slot 0, scores > 1 to slot 100001, above every threshold th <= 100000).  Then
// "score <= th / 1e5" holds exactly for the pairs of slots t <= th.  NaN (no compare holds for it): -1, counted nowhere.
__device__ __forceinline__ int cross_thr_slot(double score) {
    if (!(score > 0.0)) return score <= 0.0 ? 0 : -1;
    if (score > 1.0) return 100001;
    int t = (int)ceil(score * 1e5);                      // within 1 of the answer: the product is off by at most an ulp
    while (t > 0 && score <= (double)(t - 1) / 1e5) --t;
    while (t < 100000 && !(score <= (double)t / 1e5)) ++t;
    return t;
}

// ---- cross-matching scores (/root/reference/utils/eval.py:102-137): every unordered pair (j < i) of one embedding set, in
// the reference's order l = i (i - 1) / 2 + j; same float64-of-float32-differences arithmetic as pair_score, label 1 where
// the identities agree.  One thread per pair, 16 x 16 pairs per block.
__global__ __launch_bounds__(256) void cross_score_kernel(const float* __restrict__ e, const int64_t* __restrict__ labels, int n, int d,
                                                          double* __restrict__ scores, double* __restrict__ pair_labels,
                                                          int* __restrict__ hist_idx, int* __restrict__ hist_genuine,
                                                          int* __restrict__ hist_imposter) {
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= n || j >= i) return;
    double sum = 0.0;
    for (int k = 0; k < d; ++k) sum = cross_acc(sum, e[(size_t)j * d + k], e[(size_t)i * d + k]);
    const double score = cross_pair_score(sum);
    const int idx = cross_bin(score);
    const size_t l = (size_t)i * (i - 1) / 2 + j;
    const bool genuine = labels[j] == labels[i];
    scores[l] = score;
    pair_labels[l] = genuine ? 1.0 : 0.0;
    hist_idx[l] = idx;
    if (idx >= 0 && idx <= 100000) atomicAdd(genuine ? hist_genuine + idx : hist_imposter + idx, 1);
}

// ---- cross-matching histograms without the pair list: the pairs (i, j < i) with i in a band [i0, i1) add into four uint64
// histograms (reference bins and threshold slots, genuine / imposter).  Tiles of 128 x 128 pairs, 256 threads, each thread an
// 8 x 8 register tile of float64 sums; row slices of both blocks are staged through LDS in K-chunks of 32, [k][row] so that one
// thread's 8 rows at one k are two ds_read_b128.  Columns k >= d are zero on both sides and add exactly 0.  No MFMA: its internal
// order of sums is not the sequential one.
__device__ __forceinline__ void hist_add(unsigned long long* h, int k) {
    __hip_atomic_fetch_add(h + k, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256, 2) void cross_hist_kernel(const float* __restrict__ e, const int64_t* __restrict__ labels, int64_t n,
                                                            int d, int64_t i0, int64_t i1, unsigned long long* __restrict__ hg,
                                                            unsigned long long* __restrict__ hi, unsigned long long* __restrict__ tg,
                                                            unsigned long long* __restrict__ ti) {
    __shared__ __attribute__((aligned(16))) float li[CH_KC][CH_LD], lj[CH_KC][CH_LD];
    const int64_t ib = i0 + (int64_t)blockIdx.y * CH_T, jb = (int64_t)blockIdx.x * CH_T;
    const int64_t iend = ib + CH_T < i1 ? ib + CH_T : i1;
    if (jb >= iend - 1) return;                          // no j < i in this tile (block-uniform, before any barrier)
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
    for (int k0 = 0; k0 < d; k0 += CH_KC) {
        __syncthreads();
        for (int m = threadIdx.x; m < CH_T * CH_KC; m += 256) {
            const int r = m / CH_KC, kk = m % CH_KC, k = k0 + kk;
            const int64_t gi = ib + r, gj = jb + r;      // both < iend <= n when loaded
            li[kk][r] = (gi < iend && k < d) ? e[gi * d + k] : 0.f;
            lj[kk][r] = (gj < iend && k < d) ? e[gj * d + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < CH_KC; ++kk) {
            const f32x4_t a0 = *(const f32x4_t*)&li[kk][ty * 8], a1 = *(const f32x4_t*)&li[kk][ty * 8 + 4];
            const f32x4_t b0 = *(const f32x4_t*)&lj[kk][tx * 8], b1 = *(const f32x4_t*)&lj[kk][tx * 8 + 4];
            const float ai[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            const float bj[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[a][b] = cross_acc(acc[a][b], bj[b], ai[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int64_t i = ib + ty * 8 + a;
        if (i >= iend) continue;
        const int64_t lab = labels[i];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int64_t j = jb + tx * 8 + b;
            if (j >= i) continue;
            const double score = cross_pair_score(acc[a][b]);
            const bool genuine = labels[j] == lab;
            const int idx = cross_bin(score), t = cross_thr_slot(score);
            if (idx >= 0 && idx <= 100000) hist_add(genuine ? hg : hi, idx);
            if (t >= 0) hist_add(genuine ? tg : ti, t);
        }
    }
}
}  // namespace frhip

extern "C" int frhip_pair_score(const float* e1, const float* e2, const int64_t* labels, int n, int d, double* scores,
                                int* hist_idx, int* hist_genuine, int* hist_imposter, hipStream_t stream) {
    if (n <= 0) return FRHIP_OK;
    hipLaunchKernelGGL(frhip::pair_score_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, e1, e2, labels, n, d, scores,
                       hist_idx, hist_genuine, hist_imposter);
    return frhip::check_launch("frhip_pair_score");
}

extern "C" int frhip_cross_score(const float* e, const int64_t* labels, int n, int d, double* scores, double* pair_labels,
                                 int* hist_idx, int* hist_genuine, int* hist_imposter, hipStream_t stream) {
    if (n <= 1) return FRHIP_OK;
    if (n > 65535 * 16) { frhip::set_error("frhip_cross_score: n = %d too large", n); return FRHIP_EINVAL; }
    const int t = (n + 15) / 16;
    hipLaunchKernelGGL(frhip::cross_score_kernel, dim3(t, t), dim3(256), 0, stream, e, labels, n, d, scores, pair_labels,
                       hist_idx, hist_genuine, hist_imposter);
    return frhip::check_launch("frhip_cross_score");
}

extern "C" int frhip_cross_hist(const float* e, const int64_t* labels, int64_t n, int d, int64_t i0, int64_t i1, uint64_t* hist_genuine,
                                uint64_t* hist_imposter, uint64_t* thr_genuine, uint64_t* thr_imposter, hipStream_t stream) {
    if (n < 0 || d <= 0 || i0 < 0 || i1 > n || i0 > i1) {
        frhip::set_error("frhip_cross_hist: bad arguments n = %lld, d = %d, band [%lld, %lld)", (long long)n, d, (long long)i0,
                         (long long)i1);
        return FRHIP_EINVAL;
    }
    if (i1 < 2 || i0 == i1) return FRHIP_OK;             // no pair j < i in the band
    if (!e || !labels || !hist_genuine || !hist_imposter || !thr_genuine || !thr_imposter) {
        frhip::set_error("frhip_cross_hist: null pointer");
        return FRHIP_EINVAL;
    }
    using frhip::CH_T;
    const int64_t cols = (i1 - 2) / CH_T + 1;           // column tiles up to the last j = i1 - 2
    if (cols > 0x7fffffff / 256) { frhip::set_error("frhip_cross_hist: n = %lld too large", (long long)n); return FRHIP_EINVAL; }
    // grid.y is capped at 65535: taller bands go as several launches of at most 65535 row tiles
    for (int64_t r0 = i0; r0 < i1; r0 += (int64_t)65535 * CH_T) {
        const int64_t r1 = r0 + (int64_t)65535 * CH_T < i1 ? r0 + (int64_t)65535 * CH_T : i1;
        hipLaunchKernelGGL(frhip::cross_hist_kernel, dim3((unsigned)cols, (unsigned)((r1 - r0 + CH_T - 1) / CH_T)), dim3(256), 0, stream,
                           e, labels, n, d, r0, r1, (unsigned long long*)hist_genuine, (unsigned long long*)hist_imposter,
                           (unsigned long long*)thr_genuine, (unsigned long long*)thr_imposter);
        const int rc = frhip::check_launch("frhip_cross_hist");
        if (rc) return rc;
    }
    return FRHIP_OK;
}
