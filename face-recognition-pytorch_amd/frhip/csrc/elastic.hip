// ElasticFace (Boutros et al., CVPR-W 2022; not in the reference): every row's margin is a draw from N(m, sigma), new at every step,
// and in the "+" variants the draws are handed out by difficulty -- the row with the smallest target cosine gets the largest margin.
// Everything here sits IN FRONT of the per-row margin kernels (frhip_head_fwd_rows / _bwd_dt_rows, frhip_margin_fwd_rows / _bwd_rows):
// it only fills the two vectors of a frhip_margin_rows_t.
//   elastic_draws_kernel     counter-based Gaussian draws (Philox4x32-10 + Box-Muller in float64), one workgroup, advances the device
//                            step counter itself: no host synchronisation, capturable
//   head_target_cos_kernel   the target cosine of every row on the shard that owns it: one wavefront per row
//   elastic_rank_kernel      exact ranks by counting, of the merged cosines (descending) and of the draws (ascending, scattered into
//                            sorted order); keys stream through LDS tiles, each thread owns a row
//   elastic_pick_kernel      row i takes the sorted draw at its rank
// Definitions: frhip.h.
#include "common.h"
#include "frhip.h"

namespace frhip {

// ---- Philox4x32-10 (Salmon et al., SC 2011).  counter = (row, 0, step low, step high), key = (seed low, seed high).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& x0, uint32_t& x1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    x0 = c0; x1 = c1;                                  // x2, x3 are not used
}

// dst[i] = float(mean + sd z_i), z_i the Box-Muller value of row i's Philox output at (seed, *step); update == 0: dst[i] = float(mean).
// zero (may be null): the other vector of the pair, filled with 0.  ONE workgroup: every thread reads *step, and thread 0 writes
// step + 1 behind a barrier after the last use.
__global__ __launch_bounds__(1024) void elastic_draws_kernel(int n, double mean, double sd, long long seed, long long* __restrict__ step,
                                                             int update, float* __restrict__ dst, float* __restrict__ zero) {
    const unsigned long long st = (unsigned long long)step[0];
    const uint32_t k0 = (uint32_t)(unsigned long long)seed, k1 = (uint32_t)((unsigned long long)seed >> 32);
    const uint32_t s0 = (uint32_t)st, s1 = (uint32_t)(st >> 32);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float g = (float)mean;
        if (update) {
            uint32_t x0, x1;
            philox4x32_10((uint32_t)i, 0u, s0, s1, k0, k1, x0, x1);
            const double u1 = ((double)x0 + 0.5) * 0x1p-32, u2 = ((double)x1 + 0.5) * 0x1p-32;
            g = (float)(mean + sd * (sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2)));
        }
        dst[i] = g;
        if (zero) zero[i] = 0.f;
    }
    __syncthreads();                                   // every thread has read the old step ...
    if (update && threadIdx.x == 0) step[0] = (long long)(st + 1ull);      // ... before thread 0 overwrites it
}

// ---- target cosine: tcos[row] = max_k <ehat[row], what[k * classes + label]>, -2 where the label is -1.  One wavefront per row, four
// rows per workgroup; lane l takes the 16-byte vectors l, l + 64, ... of the row and of the centre, multiplies in fp32 and adds in
// element order, then the 64 partial sums meet in a butterfly: the order of the sum depends on d alone.
template <typename T>
__global__ __launch_bounds__(256) void head_target_cos_kernel(const T* __restrict__ ehat, const T* __restrict__ what,
                                                              const int* __restrict__ labels, int n, int classes, int d, int K,
                                                              float* __restrict__ tcos) {
    typedef Vec16<T> V;
    const int row = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = lane_id();
    if (row >= n) return;                              // wave-uniform; no barrier below
    const int lab = labels[row];
    if (lab < 0 || lab >= classes) {                   // another shard owns the row (a label past the table is treated alike: no read)
        if (lane == 0) tcos[row] = -2.f;
        return;
    }
    const int vecs = d / V::N;
    const V* e = reinterpret_cast<const V*>(ehat + (size_t)row * d);
    float best = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const V* w = reinterpret_cast<const V*>(what + ((size_t)k * classes + lab) * d);
        float acc = 0.f;
        for (int v = lane; v < vecs; v += 64) {
            const V a = e[v], b = w[v];
#pragma unroll
            for (int j = 0; j < V::N; ++j) acc = __builtin_fmaf(a.get(j), b.get(j), acc);
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, s);
        best = fmaxf(best, acc);
    }
    if (lane == 0) tcos[row] = best;
}

// ---- exact ranks by counting.  blockIdx.y == 0: key_i = max over the world_size rows of tcos (NaN counts as -2, "nobody owns it"),
// rank_i = #{j : key_j > key_i, or key_j == key_i and j < i} -> rank[i].  blockIdx.y == 1: the same count on key = -g, i.e. the position
// of g_i among the draws in ascending order, ties in index order -> sorted[position] = g_i.  The counts are a permutation of 0 .. n - 1
// whatever the values are (j == i never counts), so both stores stay inside [0, n).
constexpr int EL_TILE = 1024, EL_THREADS = 256;

__device__ __forceinline__ float elastic_key(const float* __restrict__ tcos, int ws, int n, const float* __restrict__ g, int which, int j) {
    if (which) return -g[j];
    float c = -2.f;
    for (int r = 0; r < ws; ++r) c = fmaxf(c, tcos[(size_t)r * n + j]);     // fmaxf drops a NaN operand; the sentinel is the floor
    return c;
}

__global__ __launch_bounds__(EL_THREADS) void elastic_rank_kernel(const float* __restrict__ tcos, int ws, int n, const float* __restrict__ g,
                                                                 int* __restrict__ rank, float* __restrict__ sorted) {
    __shared__ __attribute__((aligned(16))) float tile[EL_TILE];
    const int which = blockIdx.y, i = blockIdx.x * EL_THREADS + threadIdx.x;
    const bool live = i < n;
    const float mine = live ? elastic_key(tcos, ws, n, g, which, i) : 0.f;
    int count = 0;
    for (int j0 = 0; j0 < n; j0 += EL_TILE) {
        __syncthreads();                               // the previous tile has been read by everyone
#pragma unroll
        for (int t = threadIdx.x; t < EL_TILE; t += EL_THREADS)
            tile[t] = j0 + t < n ? elastic_key(tcos, ws, n, g, which, j0 + t) : -INFINITY;      // -inf behind the end: never above, never "j < i"
        __syncthreads();
        // every lane reads the same 16 bytes (a broadcast); rows before this tile win ties against all of it, rows behind it against none
        const int before = i - j0;                     // entries t < before have j < i
        const int filled = min(EL_TILE, (n - j0 + 3) & ~3);               // whole 16-byte groups up to the last key (its tail is -inf)
#pragma unroll 4
        for (int t = 0; t < filled; t += 4) {
            const f32x4_t k = *reinterpret_cast<const f32x4_t*>(&tile[t]);
#pragma unroll
            for (int q = 0; q < 4; ++q) count += (k[q] > mine || (k[q] == mine && t + q < before)) ? 1 : 0;
        }
    }
    if (!live) return;
    if (which) sorted[count] = g[i];
    else rank[i] = count;
}

__global__ __launch_bounds__(256) void elastic_pick_kernel(const int* __restrict__ rank, const float* __restrict__ sorted, int n, int kind,
                                                           float* __restrict__ m_ang, float* __restrict__ m_add) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = sorted[rank[i]];
    m_ang[i] = kind == 0 ? v : 0.f;
    m_add[i] = kind == 0 ? 0.f : v;
}

constexpr int ELASTIC_MAX_N = 65536;

static int draws_args(const char* who, int n, bool ptrs, double sd) {
    if (n < 1 || !ptrs || !(sd >= 0.0)) {
        set_error("%s: needs n >= 1 rows (n=%d), non-null step and outputs, and std >= 0 (std=%g)", who, n, sd);
        return FRHIP_EINVAL;
    }
    return FRHIP_OK;
}

}  // namespace frhip

using namespace frhip;

extern "C" int frhip_elastic_draws(int n, double mean, double std, long long seed, long long* step, int update, float* g,
                                   hipStream_t stream) {
    if (const int rc = draws_args("frhip_elastic_draws", n, step && g, std)) return rc;
    hipLaunchKernelGGL(elastic_draws_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, n, mean, std, seed, step, update, g,
                       (float*)nullptr);
    return check_launch("frhip_elastic_draws");
}

extern "C" int frhip_elastic_margins(int n, int kind, double mean, double std, long long seed, long long* step, int update, float* m_ang,
                                     float* m_add, hipStream_t stream) {
    if (const int rc = draws_args("frhip_elastic_margins", n, step && m_ang && m_add, std)) return rc;
    if (kind != 0 && kind != 1) { set_error("frhip_elastic_margins: kind %d is neither 0 (angular) nor 1 (additive)", kind); return FRHIP_EINVAL; }
    hipLaunchKernelGGL(elastic_draws_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, n, mean, std, seed, step, update,
                       kind == 0 ? m_ang : m_add, kind == 0 ? m_add : m_ang);
    return check_launch("frhip_elastic_margins");
}

extern "C" int frhip_head_target_cos(int dtype, const void* ehat, const void* what, const int* labels, int n, int classes, int d,
                                     int subcenters, float* tcos, hipStream_t stream) {
    const char* who = "frhip_head_target_cos";
    return by_dtype(dtype, who, [&](auto t) {
        typedef decltype(t) T;
        const int bke = 128 / (int)sizeof(T);              // the head's K step: the d frhip_head_fwd accepts
        if (n < 1 || classes < 1 || d < 1 || (d % bke) || subcenters < 1 || subcenters > frhip_head_sub_max() || !ehat || !what ||
            !labels || !tcos) {
            set_error("%s: needs n, classes >= 1, d a multiple of %d, 1 .. %d sub-centres and non-null pointers (n=%d classes=%d d=%d "
                      "subcenters=%d)", who, bke, frhip_head_sub_max(), n, classes, d, subcenters);
            return FRHIP_EINVAL;
        }
        hipLaunchKernelGGL(head_target_cos_kernel<T>, dim3((n + 3) / 4), dim3(256), 0, stream, (const T*)ehat, (const T*)what, labels, n,
                           classes, d, subcenters, tcos);
        return check_launch(who);
    });
}

extern "C" int frhip_elastic_assign_workspace(int n) {
    return n >= 1 && n <= ELASTIC_MAX_N ? n * (int)(sizeof(int) + sizeof(float)) : 0;
}

extern "C" int frhip_elastic_assign(const float* tcos, int world_size, int n, const float* g, int kind, float* m_ang, float* m_add,
                                    void* work, size_t work_bytes, hipStream_t stream) {
    const char* who = "frhip_elastic_assign";
    if (n < 1 || n > ELASTIC_MAX_N || world_size < 1 || (kind != 0 && kind != 1) || !tcos || !g || !m_ang || !m_add) {
        set_error("%s: needs 1 <= n <= %d rows (n=%d), world_size >= 1 (%d), kind 0 or 1 (%d) and non-null tcos, g, m_ang, m_add", who,
                  ELASTIC_MAX_N, n, world_size, kind);
        return FRHIP_EINVAL;
    }
    if (!work || ((uintptr_t)work & 3) || work_bytes < (size_t)frhip_elastic_assign_workspace(n)) {
        set_error("%s: the workspace must be 4-byte aligned and hold frhip_elastic_assign_workspace(%d) = %d bytes, got %zu", who, n,
                  frhip_elastic_assign_workspace(n), work_bytes);
        return FRHIP_EINVAL;
    }
    int* rank = (int*)work;
    float* sorted = (float*)work + n;
    hipLaunchKernelGGL(elastic_rank_kernel, dim3((n + EL_THREADS - 1) / EL_THREADS, 2), dim3(EL_THREADS), 0, stream, tcos, world_size, n, g,
                       rank, sorted);
    if (const int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(elastic_pick_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, rank, sorted, n, kind, m_ang, m_add);
    return check_launch(who);
}
