// The fp32 tile the latent scorers' kernels share (asr.hip, sv.hip): activations transposed in LDS as [k][frame], a weight block
// [k][64 outputs] next to them, products on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, one rounding
// per product).  Index math and the 64-deep product step only: staging, epilogues and launch geometry stay with the kernels.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

// element (k, frame r), r in [0, 64), of a transposed activation tile with LD floats per k: the 4-frame groups of row k are permuted by
// k, so that the 64 lanes of a transposed store (lane = k) spread over 16 banks instead of one; a thread's 4 frames stay one aligned
// 16-byte read.  (sv.hip r_at: the same permutation inside every 64-frame span of a wider tile.)
template <int LD>
__device__ __forceinline__ int tile_at(int k, int r) { return k * LD + 4 * ((r >> 2) ^ (k & 15)) + (r & 3); }

// One 32 x 32 block, 64 deep: acc += A[frame fr of this lane][k] . W[w0 + k][n0 + (l & 31)], k = 0 .. 63.  Lane l feeds A[fr][k + (l >> 5)]
// and W[w0 + k + (l >> 5)][n0 + (l & 31)], one float each (fr carries l & 31 too), both conflict-free LDS reads; the result has its column
// on the lane and its rows in the 16 registers (tile_row).  w0: the weight row of k = 0 (a tap's offset).
template <int LD>
__device__ __forceinline__ void mfma_k64(const float* aT, int fr, const float* wS, int w0, int n0, int lane, f32x16& acc) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll 8
    for (int k = 0; k < 64; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aT[tile_at<LD>(k + h, fr)], wS[(w0 + k + h) * 64 + n0 + r], acc, 0, 0, 0);
}

// row of the 32 x 32 block that register i of the accumulator holds on this lane
__device__ __forceinline__ int tile_row(int i, int lane) { return 4 * (lane >> 5) + (i & 3) + 8 * (i >> 2); }

// frames of batch row b, clamped into [0, N]
__device__ __forceinline__ int row_len(const int* n_len, int b, int N) {
    const int n = n_len[b];
    return n < 0 ? 0 : n > N ? N : n;
}

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }   // (host: workspace carve-outs)
