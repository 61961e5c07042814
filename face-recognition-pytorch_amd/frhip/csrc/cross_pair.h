// frhip -- the per-pair arithmetic of the cross test, shared by cross_score_kernel (pair list), cross_hist_kernel (histograms
// only) and gallery_topk_kernel (1:N search) so that the routes cannot drift apart.
#pragma once
#include "common.h"

namespace frhip {

// sum += (double)(float)(e[j][k] - e[i][k])^2 in ascending k: the square of a float is exact in double (48 significant bits fit
// in 53), so a fused or a separate multiply-add give the same sum and only the order of the adds matters.
__device__ __forceinline__ double cross_acc(double sum, float ej, float ei) {
    const double dd = (double)(ej - ei);
    return sum + dd * dd;
}
__device__ __forceinline__ double cross_pair_score(double sum) { return 1.0 - sum / 4.0; }

// tile shape of the register-tile kernels: 128 x 128 pairs per 256-thread workgroup, an 8 x 8 tile of float64 sums per thread,
// row slices of both sides staged through LDS in K-chunks of 32 as [k][row] (+ 4 floats of padding per k)
constexpr int CH_T = 128, CH_KC = 32, CH_LD = CH_T + 4;

}  // namespace frhip
