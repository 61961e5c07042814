// frhip -- 1:N identification: for every probe row the k best gallery rows under the cross test's score, without ever
// writing the P x G score matrix.  gfx950 only.
//
// Two launches per call.  gallery_topk_kernel: the cross_hist register tile (128 x 128 pairs per 256-thread workgroup, 8 x 8
// float64 sums per thread, both row slices staged through LDS in K-chunks of 32) over the gallery tiles s, s + S, s + 2 S, ... of
// one probe tile; the S workgroups of a probe tile ("splits") each keep a sorted k-list per probe row in the workspace, with only
// the k-th best (score, index) of every row in LDS.  The tile epilogue compares each pair against that threshold; the few that
// beat it go through per-row LDS slots to the thread that owns the row, which inserts them into its list.  gallery_topk_merge_kernel:
// one wave per probe row selects the k best of the S split lists and the list already in top_score / top_index.
// The order is total (score descending, then gallery index ascending), so the result depends neither on S nor on the tile order.
#include "common.h"
#include "cross_pair.h"
#include "frhip.h"

#include <math.h>

namespace frhip {

constexpr int GT_SLOTS = 8;                    // candidates one probe row takes per epilogue round (LDS)
constexpr int GT_MAX_D = 1 << 27;               // 32-bit lane offsets while staging: 7 d + 31 < 2^30
constexpr int GT_WG_TARGET = 1024;             // split workgroups the workspace is sized for (or one per probe tile, if more)

// (s, j) comes before (ts, tj) in the order of the lists: higher score first, equal scores by ascending gallery index.  tj < 0
// marks an unfilled slot, which everything with a valid index precedes.  No compare holds for a NaN score: never a candidate.
__device__ __forceinline__ bool gt_before(double s, int64_t j, double ts, int64_t tj) {
    return s > ts || (s == ts && (tj < 0 || j < tj));
}

__global__ __launch_bounds__(256, 2) void gallery_topk_kernel(const float* __restrict__ probe, const float* __restrict__ gallery,
                                                              const int64_t* __restrict__ exclude, int64_t np, int d, int k,
                                                              int64_t g0, int64_t g1, int splits, double* __restrict__ ws_score,
                                                              int64_t* __restrict__ ws_index) {
    __shared__ __attribute__((aligned(16))) float li[CH_KC][CH_LD], lj[CH_KC][CH_LD];
    __shared__ double thr_s[CH_T], q_score[CH_T][GT_SLOTS];
    __shared__ int64_t thr_i[CH_T], excl[CH_T];
    __shared__ int q_col[CH_T][GT_SLOTS], q_cnt[CH_T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int split = (int)(blockIdx.x % (unsigned)splits);
    const int64_t ib = (int64_t)(blockIdx.x / (unsigned)splits) * CH_T;
    const int64_t iend = ib + CH_T < np ? ib + CH_T : np;
    const int ni = (int)(iend - ib), kk = tid & (CH_KC - 1), r0 = tid / CH_KC;
    const unsigned voff = (unsigned)r0 * (unsigned)d + (unsigned)kk;
    // this workgroup's lists: [row of the tile][k], written here before anything reads them
    double* const my_s = ws_score + ((size_t)blockIdx.x * CH_T + (tid & (CH_T - 1))) * k;
    int64_t* const my_i = ws_index + ((size_t)blockIdx.x * CH_T + (tid & (CH_T - 1))) * k;
    const bool owner = tid < CH_T && ib + tid < iend;          // thread r owns probe row ib + r: the only one to touch its list
    if (tid < CH_T) {
        if (owner)
            for (int p = 0; p < k; ++p) { my_s[p] = -INFINITY; my_i[p] = -1; }
        thr_s[tid] = owner ? -INFINITY : INFINITY;             // rows past the last probe never see a candidate
        thr_i[tid] = owner ? -1 : 0;
        excl[tid] = (owner && exclude) ? exclude[ib + tid] : -1;
    }
    const int64_t tiles = (g1 - g0 + CH_T - 1) / CH_T;
    for (int64_t t = split; t < tiles; t += splits) {
        const int64_t jb = g0 + t * CH_T, jend = jb + CH_T < g1 ? jb + CH_T : g1;
        double acc[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
        const int nj = (int)(jend - jb);
        for (int k0 = 0; k0 < d; k0 += CH_KC) {
            __syncthreads();
            // thread (r0, kk) stages column k0 + kk of rows r0, r0 + 8, ...: a wave reads two 128-byte row pieces per load.  The
            // row base is workgroup-uniform and the lane offset 32 bits (7 d + 31 < 2^30), so no 64-bit address lives per load
#pragma unroll 4
            for (int it = 0; it < CH_T / 8; ++it) {
                const int r = it * 8 + r0;
                const float* pi_ = probe + (ib + it * 8) * d + k0;
                const float* pj_ = gallery + (jb + it * 8) * d + k0;
                li[kk][r] = (r < ni && k0 + kk < d) ? pi_[voff] : 0.f;
                lj[kk][r] = (r < nj && k0 + kk < d) ? pj_[voff] : 0.f;
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
        // ---- epilogue: which of this thread's 64 pairs reach their row's k-th best score?  One compare per pair; ties with the
        // threshold are settled by index below.  (thresholds: last written before the barriers of the K loop above)
        unsigned half[2] = {0u, 0u};                           // bit a * 8 + b, shifted in from the top: no mask constants
#pragma unroll
        for (int a = 7; a >= 0; --a) {
            const double ts = thr_s[ty * 8 + a];
#pragma unroll
            for (int b = 7; b >= 0; --b) {
                acc[a][b] = cross_pair_score(acc[a][b]);         // the sums become the scores, in place
                half[a >> 2] = (half[a >> 2] << 1) | (acc[a][b] >= ts ? 1u : 0u);
            }
        }
        unsigned long long pend = (unsigned long long)half[1] << 32 | half[0];
        if (!__syncthreads_or(pend != 0)) continue;            // nearly every tile after the first few
        // rounds: every row takes up to GT_SLOTS candidates, its owner inserts them, what is left is filtered against the new
        // thresholds and goes into the next round
        for (;;) {
            if (tid < CH_T) q_cnt[tid] = 0;
            __syncthreads();                                     // counts zeroed, thresholds of the last round written
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                unsigned m8 = (unsigned)(pend >> (a * 8)) & 0xffu, left = 0;
                if (m8 == 0) continue;
                const int row = ty * 8 + a;
                const double ts = thr_s[row];
                const int64_t ti = thr_i[row], ex = excl[row];
                bool full = false;
                while (m8) {
                    const int b = __builtin_ctz(m8);
                    m8 &= m8 - 1;
                    double sc = acc[a][0];                       // select chain: no dynamic register index
#pragma unroll
                    for (int c = 1; c < 8; ++c) sc = b == c ? acc[a][c] : sc;
                    const int col = tx * 8 + b;
                    const int64_t j = jb + col;
                    if (col >= nj || j == ex || !gt_before(sc, j, ts, ti)) continue;
                    const int pos = full ? GT_SLOTS : atomicAdd(&q_cnt[row], 1);
                    if (pos >= GT_SLOTS) { full = true; left |= 1u << b; continue; }
                    q_score[row][pos] = sc;
                    q_col[row][pos] = col;
                }
                pend = (pend & ~(0xffull << (a * 8))) | ((unsigned long long)left << (a * 8));
            }
            const int more = __syncthreads_or(pend != 0);
            if (owner) {
                const int n = q_cnt[tid] < GT_SLOTS ? q_cnt[tid] : GT_SLOTS;
                double ts = thr_s[tid];
                int64_t ti = thr_i[tid];
                for (int q = 0; q < n; ++q) {
                    const double s = q_score[tid][q];
                    const int64_t j = jb + q_col[tid][q];
                    if (!gt_before(s, j, ts, ti)) continue;     // the threshold moved since the push
                    int lo = 0, hi = k - 1;                      // the slot it takes: the first entry it comes before
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (gt_before(s, j, my_s[mid], my_i[mid])) hi = mid; else lo = mid + 1;
                    }
                    int p = k - 1;
                    for (; p - lo >= 4; p -= 4) {                // the tail moves down one slot, four loads in flight
                        const double s0 = my_s[p - 1], s1 = my_s[p - 2], s2 = my_s[p - 3], s3 = my_s[p - 4];
                        const int64_t i0 = my_i[p - 1], i1 = my_i[p - 2], i2 = my_i[p - 3], i3 = my_i[p - 4];
                        my_s[p] = s0; my_s[p - 1] = s1; my_s[p - 2] = s2; my_s[p - 3] = s3;
                        my_i[p] = i0; my_i[p - 1] = i1; my_i[p - 2] = i2; my_i[p - 3] = i3;
                    }
                    for (; p > lo; --p) { my_s[p] = my_s[p - 1]; my_i[p] = my_i[p - 1]; }
                    my_s[lo] = s;
                    my_i[lo] = j;
                    ts = my_s[k - 1];
                    ti = my_i[k - 1];
                }
                thr_s[tid] = ts;
                thr_i[tid] = ti;
            }
            if (!more) break;                                    // block-uniform; the next barrier is the K loop's
        }
    }
}

// one wave per probe row: the k first entries, in the order of the lists, of the union of the row's `splits` workspace lists and
// the list already in top_score / top_index.  Every list is sorted, so round r finds in each list the first entry behind the
// entry chosen in round r - 1 by bisection, lanes take the best over their lists and a butterfly takes the best over the lanes.
// An entry present in two lists (a band merged twice) is chosen once.  Lane r keeps the r-th choice; the row is written at the end.
__global__ __launch_bounds__(64) void gallery_topk_merge_kernel(const double* __restrict__ ws_score, const int64_t* __restrict__ ws_index,
                                                                int splits, int k, double* top_score, int64_t* top_index) {
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const size_t tile = (size_t)(row / CH_T), r = (size_t)(row % CH_T);
    double prev_s = 0.0, keep_s = -INFINITY;
    int64_t prev_i = -1, keep_i = -1;
    for (int round = 0; round < k; ++round) {
        double best_s = -INFINITY;
        int64_t best_i = -1;
        for (int l = lane; l <= splits; l += 64) {
            const double* ls = l < splits ? ws_score + ((tile * splits + l) * CH_T + r) * k : top_score + (size_t)row * k;
            const int64_t* lx = l < splits ? ws_index + ((tile * splits + l) * CH_T + r) * k : top_index + (size_t)row * k;
            int lo = 0, hi = round ? k : 0;
            while (lo < hi) {                                    // first entry behind prev (unfilled slots count as behind)
                const int mid = (lo + hi) >> 1;
                const int64_t mi = lx[mid];
                if (mi < 0 || gt_before(prev_s, prev_i, ls[mid], mi)) hi = mid; else lo = mid + 1;
            }
            if (lo < k) {
                const double s = ls[lo];
                const int64_t j = lx[lo];
                if (j >= 0 && gt_before(s, j, best_s, best_i)) { best_s = s; best_i = j; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double os = __shfl_xor(best_s, m);
            const int ol = __shfl_xor((int)(uint32_t)best_i, m), oh = __shfl_xor((int)(best_i >> 32), m);
            const int64_t oi = (int64_t)(((uint64_t)(uint32_t)oh << 32) | (uint32_t)ol);
            if (oi >= 0 && gt_before(os, oi, best_s, best_i)) { best_s = os; best_i = oi; }
        }
        if (best_i < 0) break;                                   // wave-uniform: the lists are exhausted
        if (lane == round) { keep_s = best_s; keep_i = best_i; }
        prev_s = best_s;
        prev_i = best_i;
    }
    __syncthreads();                                             // every read of the old row is done
    if (lane < k) {
        top_score[(size_t)row * k + lane] = keep_s;
        top_index[(size_t)row * k + lane] = keep_i;
    }
}

// workgroups that run at the same time on the device: occupancy of the search kernel x compute units
static int gt_slots() {
    static const int per_cu = [] {                              // a property of the code object: asked once
        int n = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gallery_topk_kernel, 256, 0) == hipSuccess && n >= 1 ? n : 2;
    }();
    return per_cu * device_cu_count();
}

// splits of the gallery band per probe tile: the S <= cap that minimises waves-of-workgroups x (tiles per workgroup + 1); the
// + 1 is the first tile of a workgroup, whose epilogue fills the lists from nothing
static int gt_splits(int64_t ptiles, int64_t gtiles, int64_t cap, int slots) {
    if (cap > gtiles) cap = gtiles;
    if (cap > 65536) cap = 65536;
    int64_t best = 1, best_cost = -1;
    for (int64_t s = 1; s <= cap; ++s) {
        const int64_t cost = ((ptiles * s + slots - 1) / slots) * ((gtiles + s - 1) / s + 1);
        if (best_cost < 0 || cost < best_cost) { best = s; best_cost = cost; }
    }
    return (int)best;
}

}  // namespace frhip

static size_t gt_workspace_bytes(int64_t p, int k) {
    const int64_t ptiles = (p + frhip::CH_T - 1) / frhip::CH_T;
    const int64_t wgs = ptiles > frhip::GT_WG_TARGET ? ptiles : frhip::GT_WG_TARGET;
    return (size_t)wgs * frhip::CH_T * (size_t)k * (sizeof(double) + sizeof(int64_t));
}

extern "C" int frhip_gallery_topk_workspace(int64_t p, int k, int64_t* bytes) {
    if (p < 0 || k < 1 || k > 64 || !bytes) {
        frhip::set_error("frhip_gallery_topk_workspace: bad arguments p = %lld, k = %d%s", (long long)p, k, bytes ? "" : ", null pointer");
        return FRHIP_EINVAL;
    }
    *bytes = p == 0 ? 0 : (int64_t)gt_workspace_bytes(p, k);
    return FRHIP_OK;
}

extern "C" int frhip_gallery_topk(const float* probe, const float* gallery, const int64_t* exclude, int64_t p, int64_t g, int d, int k,
                                  int64_t g0, int64_t g1, double* top_score, int64_t* top_index, void* workspace,
                                  size_t workspace_bytes, hipStream_t stream) {
    if (p < 0 || g < 0 || d <= 0 || d > frhip::GT_MAX_D || k < 1 || k > 64 || g0 < 0 || g1 > g || g0 > g1) {
        frhip::set_error("frhip_gallery_topk: bad arguments p = %lld, g = %lld, d = %d (1..2^27), k = %d (1..64), band [%lld, %lld)", (long long)p,
                         (long long)g, d, k, (long long)g0, (long long)g1);
        return FRHIP_EINVAL;
    }
    if (p == 0 || g0 == g1) return FRHIP_OK;                     // no probe, or an empty band: the lists stay as they are
    if (!probe || !gallery || !top_score || !top_index || !workspace) {
        frhip::set_error("frhip_gallery_topk: null pointer");
        return FRHIP_EINVAL;
    }
    using frhip::CH_T;
    const int64_t ptiles = (p + CH_T - 1) / CH_T, gtiles = (g1 - g0 + CH_T - 1) / CH_T;
    const size_t per_wg = (size_t)CH_T * k * (sizeof(double) + sizeof(int64_t));
    const int64_t cap = (int64_t)(workspace_bytes / per_wg / (size_t)ptiles);
    if (p > 0x7fffffff) { frhip::set_error("frhip_gallery_topk: p = %lld too large", (long long)p); return FRHIP_EINVAL; }
    if (cap < 1) {
        frhip::set_error("frhip_gallery_topk: workspace of %zu bytes is too small for p = %lld, k = %d (frhip_gallery_topk_workspace: %zu)",
                         workspace_bytes, (long long)p, k, gt_workspace_bytes(p, k));
        return FRHIP_EINVAL;
    }
    const int64_t budget = frhip::GT_WG_TARGET / ptiles;         // keeps the split lists within the queried workspace size
    const int splits = frhip::gt_splits(ptiles, gtiles, cap < budget ? cap : (budget < 1 ? 1 : budget), frhip::gt_slots());
    const size_t wgs = (size_t)ptiles * splits;                 // <= max(ptiles, GT_WG_TARGET)
    double* ws_score = (double*)workspace;
    int64_t* ws_index = (int64_t*)(ws_score + wgs * CH_T * k);
    hipLaunchKernelGGL(frhip::gallery_topk_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, probe, gallery, exclude, p, d, k, g0, g1,
                       splits, ws_score, ws_index);
    int rc = frhip::check_launch("frhip_gallery_topk");
    if (rc) return rc;
    hipLaunchKernelGGL(frhip::gallery_topk_merge_kernel, dim3((unsigned)p), dim3(64), 0, stream, ws_score, ws_index, splits, k, top_score,
                       top_index);
    return frhip::check_launch("frhip_gallery_topk (merge)");
}
