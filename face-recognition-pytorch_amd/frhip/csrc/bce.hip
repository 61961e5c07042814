// The sigmoid (binary cross-entropy) head, UniFace / SphereFace2 (not in the reference): what sits BEHIND the head's MG_BCE variant
// (head.hip) -- the fold of its per-group partials into rows, the rank's pair and the cross-rank merge -- and the explicit-logit pair
// of the stand-alone module.  The element rules are margin_shared.h's, shared with the fused head.  Definitions: frhip.h.
#include "common.h"
#include "margin_shared.h"
#include "frhip.h"

namespace frhip {

// the sum of v over the workgroup, on every thread: butterfly inside a wavefront, then the wavefronts' sums in index order
__device__ __forceinline__ double bce_block_sum(double v, double* red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    __syncthreads();                                    // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
    return r;
}

// one thread per row: the groups' partials in group order, float64.  groups x n elements: a few MB at 122 000 classes.
__global__ __launch_bounds__(256) void bce_rowfold_kernel(const float* __restrict__ part_loss, const float* __restrict__ part_db,
                                                          int groups, int n, float* __restrict__ rowloss, float* __restrict__ rowdb) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    double l = 0.0, b = 0.0;
    for (int g = 0; g < groups; ++g) {
        l += (double)part_loss[(size_t)g * n + m];
        b += (double)part_db[(size_t)g * n + m];
    }
    rowloss[m] = (float)l;
    rowdb[m] = (float)b;
}

// ONE workgroup: each thread its rows i = tid, tid + blockDim, ... in that order, then the block sum: the order depends on n alone
__global__ __launch_bounds__(1024) void bce_reduce_kernel(const float* __restrict__ rowloss, const float* __restrict__ rowdb, int n,
                                                          float* __restrict__ pair) {
    __shared__ double red[16];
    double l = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) { l += (double)rowloss[i]; b += (double)rowdb[i]; }
    l = bce_block_sum(l, red);
    b = bce_block_sum(b, red);
    if (threadIdx.x == 0) { pair[0] = (float)l; pair[1] = (float)b; }
}

// one thread: world_size pairs in rank order, float64, scaled by 1 / n_global once
__global__ void bce_merge_kernel(const float* __restrict__ gathered, int ws, double inv_n, float* __restrict__ loss,
                                 float* __restrict__ dbias) {
    if (threadIdx.x || blockIdx.x) return;
    double l = 0.0, b = 0.0;
    for (int r = 0; r < ws; ++r) { l += (double)gathered[2 * r]; b += (double)gathered[2 * r + 1]; }
    loss[0] = (float)(l * inv_n);
    dbias[0] = (float)(b * inv_n);
}

// one 256-thread block per row of explicit cosines
__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int C,
                                                      MarginBce mc, float* __restrict__ rowloss, float* __restrict__ rowdb) {
    __shared__ double red[4];
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    const float b = mc.bias[0];
    double l = 0.0, g = 0.0;
    for (int j = threadIdx.x; j < C; j += 256) {
        const float c = fminf(fmaxf(logits[(size_t)row * C + j], -1.f), 1.f);
        float a, dcos, db;
        const float term = j == lab ? bce_target(c, mc, b, a, dcos, db) : bce_negative(c, mc, b, a, dcos, db);
        l += (double)term;
        g += (double)db;
    }
    l = bce_block_sum(l, red);
    g = bce_block_sum(g, red);
    if (threadIdx.x == 0) { rowloss[row] = (float)l; rowdb[row] = (float)g; }
}

__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int C,
                                                      MarginBce mc, float gscale, const float* __restrict__ upstream,
                                                      float* __restrict__ gin) {
    const int row = blockIdx.x;
    const int64_t lab = labels[row];
    const float b = mc.bias[0];
    if (upstream) gscale *= upstream[0];
    for (int j = threadIdx.x; j < C; j += 256) {
        const float raw = logits[(size_t)row * C + j], c = fminf(fmaxf(raw, -1.f), 1.f);
        float a, dcos, db;
        if (j == lab) bce_target(c, mc, b, a, dcos, db);
        else bce_negative(c, mc, b, a, dcos, db);
        gin[(size_t)row * C + j] = (raw >= -1.f && raw <= 1.f) ? dcos * gscale : 0.f;
    }
}

int bce_rowfold_launch(const float* part_loss, const float* part_db, int groups, int n, float* rowloss, float* rowdb, hipStream_t stream,
                       const char* who) {
    hipLaunchKernelGGL(bce_rowfold_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, part_loss, part_db, groups, n, rowloss, rowdb);
    char tag[64];
    snprintf(tag, sizeof(tag), "%s/rowfold", who);
    return check_launch(tag);
}

}  // namespace frhip

using namespace frhip;

extern "C" int frhip_bce_reduce(const float* rowloss, const float* rowdb, int n, float* pair, hipStream_t stream) {
    if (n < 1 || !rowloss || !rowdb || !pair) {
        set_error("frhip_bce_reduce: needs n >= 1 rows (n=%d) and non-null rowloss, rowdb, pair", n);
        return FRHIP_EINVAL;
    }
    hipLaunchKernelGGL(bce_reduce_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, rowloss, rowdb, n, pair);
    return check_launch("frhip_bce_reduce");
}

extern "C" int frhip_bce_merge(const float* gathered, int world_size, int n_global, float* loss, float* dbias, hipStream_t stream) {
    if (world_size < 1 || n_global < 1 || !gathered || !loss || !dbias) {
        set_error("frhip_bce_merge: needs world_size >= 1 (%d), n_global >= 1 (%d) and non-null gathered, loss, dbias", world_size,
                  n_global);
        return FRHIP_EINVAL;
    }
    hipLaunchKernelGGL(bce_merge_kernel, dim3(1), dim3(64), 0, stream, gathered, world_size, 1.0 / (double)n_global, loss, dbias);
    return check_launch("frhip_bce_merge");
}

static int bce_args(const char* who, const frhip_margin_bce_t* mg, int n, int c, bool ptrs) {
    if (const char* why = margin_bce_desc_error(mg)) { set_error("%s: bad BCE descriptor: %s", who, why); return FRHIP_EINVAL; }
    if (n < 1 || c < 1 || !ptrs) {
        set_error("%s: needs n >= 1, c >= 1 (n=%d c=%d) and non-null operands", who, n, c);
        return FRHIP_EINVAL;
    }
    return FRHIP_OK;
}

extern "C" int frhip_bce_fwd(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_bce_t* margin, float* rowloss,
                             float* rowdb, hipStream_t stream) {
    if (const int rc = bce_args("frhip_bce_fwd", margin, n, c, logits && labels && rowloss && rowdb)) return rc;
    hipLaunchKernelGGL(bce_fwd_kernel, dim3(n), dim3(256), 0, stream, logits, labels, c, margin_bce(margin), rowloss, rowdb);
    return check_launch("frhip_bce_fwd");
}

extern "C" int frhip_bce_bwd(const float* logits, const int64_t* labels, int n, int c, const frhip_margin_bce_t* margin, float gscale,
                             const float* upstream, float* gin, hipStream_t stream) {
    if (const int rc = bce_args("frhip_bce_bwd", margin, n, c, logits && labels && gin)) return rc;
    hipLaunchKernelGGL(bce_bwd_kernel, dim3(n), dim3(256), 0, stream, logits, labels, c, margin_bce(margin), gscale, upstream, gin);
    return check_launch("frhip_bce_bwd");
}
