// frhip -- the transposing LDS fragment read shared by the weight-gradient kernels (igemm_tn.hip) and the fused stem (stem_fused.hip).
// [pixel][channel] LDS tiles of RB-byte rows are read as K = pixel MFMA fragments: 16-byte chunks are XOR-swizzled per row so that
// the transposing read ds_read_b64_tr_b16 / the strided f32 reads are bank-conflict free.
#pragma once
#include "common.h"

namespace frhip {

template <int RB> __device__ __forceinline__ int tn_swz(int row);
template <> __device__ __forceinline__ int tn_swz<256>(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
template <> __device__ __forceinline__ int tn_swz<128>(int row) { return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1; }

// fragment for one MFMA K group from a [pixel][channel] LDS tile, channels c0..c0+15, pixel rows r0 + (k slots)
template <typename T, int RB> struct TnFrag;
template <int RB> struct TnFrag<bf16_t, RB> {
    // 32 pixels per MFMA: lane group g covers pixels r0 + 8g .. 8g+7 via two transposed 4x16 block reads
    static constexpr int KROWS = 32;
    __device__ static __forceinline__ bf16x8_t load(const char* tile, int r0, int c0, int lane) {
        const int g = lane >> 4, j = lane & 15, q = j >> 2, p = j & 3;
        const int chunk = (c0 >> 3) + (p >> 1);
        const int row_a = r0 + 8 * g + q, row_b = row_a + 4;
        const char* pa = tile + row_a * RB + ((chunk ^ tn_swz<RB>(row_a)) << 4) + 8 * (p & 1);
        const char* pb = tile + row_b * RB + ((chunk ^ tn_swz<RB>(row_b)) << 4) + 8 * (p & 1);
        i16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4_t*)LDS_ADDR(pa));
        i16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4_t*)LDS_ADDR(pb));
        typedef __attribute__((ext_vector_type(8))) short i16x8_t;
        i16x8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8_t, v);
    }
};
template <int RB> struct TnFrag<float, RB> {
    // 16 pixels per "K group" (4 MFMA 16x16x4): element e of lane group g is pixel r0 + 4e + g
    static constexpr int KROWS = 16;
    __device__ static __forceinline__ f32x4_t load(const char* tile, int r0, int c0, int lane) {
        const int g = lane >> 4, i = lane & 15;
        const int col = c0 + i, chunk = col >> 2, within = (col & 3) * 4;
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = r0 + 4 * e + g;
            v[e] = *reinterpret_cast<const float*>(tile + row * RB + ((chunk ^ tn_swz<RB>(row)) << 4) + within);
        }
        return v;
    }
};

}  // namespace frhip
