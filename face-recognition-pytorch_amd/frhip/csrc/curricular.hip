// CurricularFace (Huang et al., CVPR 2020; not in the reference): what sits IN FRONT of the head's MG_CURR variant (head.hip) and the
// explicit-logit pair (margin.hip).  One small kernel turns the ranks' target cosines (frhip_head_target_cos) into the per-row
// thresholds cos(theta_y + m) and advances the running mean t of the target cosines.  Definitions: frhip.h.
#include "common.h"
#include "frhip.h"

namespace frhip {

// the sum of v over the workgroup, on every thread: butterfly inside a wavefront, then the wavefronts' sums in index order
__device__ __forceinline__ double curr_block_sum(double v, double* red) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    __syncthreads();                                    // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
    return r;
}

// c_i = max over the ws rows of tcos, from the floor -2 (fmaxf drops a NaN operand: "nobody owns it"); owned where c_i > -2, then clamped
__device__ __forceinline__ float curr_row_cos(const float* __restrict__ tcos, int ws, int n, int i, bool& owned) {
    float c = -2.f;
    for (int r = 0; r < ws; ++r) c = fmaxf(c, tcos[(size_t)r * n + i]);
    owned = c > -2.f;
    return fminf(fmaxf(c, -1.f), 1.f);
}

// ONE workgroup.  thr[i] = float(c_i cos_m - sqrt(1 - c_i^2) sin_m) in float64, 2 for a row nobody owns.  The owned cosines and their
// number are summed in float64, each thread its rows i = tid, tid + blockDim, ... in that order: the order depends on n alone (the block
// size does).  Every thread reads the old t before the first barrier; thread 0 writes the new one behind the last.
__global__ __launch_bounds__(1024) void curricular_rows_kernel(const float* __restrict__ tcos, int ws, int n, double cos_m, double sin_m,
                                                               double alpha, int update, float* __restrict__ t, float* __restrict__ thr) {
    __shared__ double red[16];
    const double t_old = update ? (double)t[0] : 0.0;
    double acc = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        bool owned;
        const double c = (double)curr_row_cos(tcos, ws, n, i, owned);
        thr[i] = owned ? (float)(c * cos_m - sqrt((1.0 - c) * (1.0 + c)) * sin_m) : 2.f;
        if (owned) { acc += c; cnt += 1.0; }
    }
    if (!update) return;                                // uniform: no thread reaches the barriers below
    const double sum = curr_block_sum(acc, red), rows = curr_block_sum(cnt, red);
    if (threadIdx.x == 0 && rows > 0.0) t[0] = (float)(alpha * (sum / rows) + (1.0 - alpha) * t_old);
}

}  // namespace frhip

using namespace frhip;

extern "C" int frhip_curricular_rows(const float* tcos, int world_size, int n, double m, double alpha, int update, float* t, float* thr,
                                     hipStream_t stream) {
    const char* who = "frhip_curricular_rows";
    const double pi = 3.14159265358979323846;
    if (n < 1 || world_size < 1) {
        set_error("%s: needs n >= 1 rows (n=%d) and world_size >= 1 (world_size=%d)", who, n, world_size);
        return FRHIP_EINVAL;
    }
    if (!tcos || !t || !thr) {
        set_error("%s: needs non-null %s", who, !tcos ? "tcos" : !t ? "t" : "thr");
        return FRHIP_EINVAL;
    }
    if (!(m >= 0.0 && m < pi)) { set_error("%s: the margin m=%g lies outside [0, pi)", who, m); return FRHIP_EINVAL; }
    if (!(alpha >= 0.0 && alpha <= 1.0)) { set_error("%s: the momentum alpha=%g lies outside [0, 1]", who, alpha); return FRHIP_EINVAL; }
    hipLaunchKernelGGL(curricular_rows_kernel, dim3(1), dim3(n > 256 ? 1024 : 256), 0, stream, tcos, world_size, n, cos(m), sin(m), alpha,
                       update, t, thr);
    return check_launch(who);
}
