// Takes: sample every row K times, keep the best-aligned one on the device (DESIGN '8d. Takes'), gfx950.
//
// take_scores: behind align_path, one workgroup of 256 threads per sampler row.  From the tapped text mass (B, N, P), the path's spans
// (B, P, 2) and its cost it counts four integer features of the row's window (frames [0, n), tokens [p0, p1), clamped as align_path
// clamps them) and folds them into one fp32 total, lower = better:
//   cells    sum over the tokens of their span length          (a monotone path has n + Pw - 1 of them at most)
//   skipped  tokens no frame of whose span attends to them     (no mass[f][p] >= tau_tok, f in the span)
//   longest  the longest span                                  (a droning phoneme)
//   idle     frames that attend to no token of the window      (no mass[f][p] >= tau_frm, p in [p0, p1))
// Every feature is a count or a maximum of integers decided by comparisons on single fp32 values (a NaN satisfies none), so no
// reduction order can change it.  Loads: thread = token walking down its span (adjacent lanes read adjacent floats of a mass row), then
// wave = frame with lanes across the tokens; nothing strides by P.  One thread folds the total from single correctly rounded fp32
// operations in a fixed order (rn_* below): a numpy float32 restatement gives feat and total bit for bit.
//
// take_select: rows are piece-major, row = g * K + k.  Grid (chunks, G); every workgroup re-derives its group's winner from the K
// totals (lowest k with the smallest key, key = NaN ? +inf : total; strict < walking k upward) and copies its chunk of the winning
// row of x (N, 64), spans (P, 2) and mass (N, P) to row g of the outputs, in 16-byte lanes where the row's byte count and both bases
// allow and in 4-byte elements otherwise.  The winner index leaves a bounded loop: in range whatever the totals hold.
// Plain VALU + LDS, no atomics: two runs return the same bits whatever else the chip is doing.
#include <algorithm>

#include "kernels.hpp"
#include "prof.hpp"
#include "row_copy.hpp"

namespace {

constexpr int TK_MAXN = 225, TK_MAXP = 198, TK_NT = 256;   // align_path's range

// Single correctly rounded fp32 operations.  HIP's __fmul_rn / __fadd_rn / __fdiv_rn are a plain product, sum and quotient in this
// toolchain, which the compiler may contract into an fma once they are inlined.  The pragma sits inside each body, so it ends with
// the body and leaves the mode of everything else in this unit to the build.  It binds while the compiler honours pragmas, which is
// hipcc's default (-ffp-contract=fast-honor-pragmas); a build that passes plain -ffp-contract=fast overrides every pragma and may fuse
// them again: tests/test_takes_gpu.py, which holds the total to numpy bit for bit, is what would say so.
__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rn_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

__global__ __launch_bounds__(TK_NT) void take_scores_kernel(const float* __restrict__ mass, const int* __restrict__ spans,
                                                            const float* __restrict__ path_score, const int* __restrict__ n_len,
                                                            const int* __restrict__ p0a, const int* __restrict__ p1a, int N, int P,
                                                            float tau_tok, float tau_frm, float w0, float w1, float w2, float w3,
                                                            int* __restrict__ feat, float* __restrict__ total) {
    __shared__ int part[4][TK_NT / 64];   // per wave: cells, skipped, longest, idle
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int nb = n_len[b], p0 = p0a[b], p1 = p1a[b];
    nb = nb < 0 ? 0 : nb > N ? N : nb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int Pw = p1 - p0;
    if (nb <= 0 || Pw <= 0) {   // (uniform)
        if (t < 4) feat[(long)b * 4 + t] = 0;
        if (t == 0) total[b] = INFINITY;
        return;
    }
    const float* const mrow = mass + (long)b * N * P;   // every index below: frame in [0, nb) <= N, token in [p0, p1) <= P
    // thread = token: its span length and whether any frame of the span attends to it
    int len = 0, skip = 0;
    if (t < Pw) {
        const int p = p0 + t;
        int first = spans[((long)b * P + p) * 2], last = spans[((long)b * P + p) * 2 + 1];
        skip = 1;
        if (first >= 0 && last >= first) {
            first = first > nb - 1 ? nb - 1 : first;   // (first >= 0 already)
            last = last > nb - 1 ? nb - 1 : last;
            len = last - first + 1;
            for (int f = first; f <= last; ++f)
                if (mrow[(long)f * P + p] >= tau_tok) skip = 0;
        }
    }
    // wave = frame, lanes across the window's tokens
    int idle = 0;
    for (int f = w; f < nb; f += TK_NT / 64) {
        int hit = 0;
        for (int q = lane; q < Pw; q += 64)
            if (mrow[(long)f * P + p0 + q] >= tau_frm) hit = 1;
        if (__ballot(hit) == 0ull) ++idle;   // (the same count in every lane of the wave)
    }
    const int cells_w = wave_sum(len), skip_w = wave_sum(skip), long_w = wave_max(len);
    if (lane == 0) { part[0][w] = cells_w; part[1][w] = skip_w; part[2][w] = long_w; part[3][w] = idle; }
    __syncthreads();
    if (t == 0) {
        int cells = 0, skipped = 0, longest = 0, idles = 0;
        for (int i = 0; i < TK_NT / 64; ++i) {
            cells += part[0][i]; skipped += part[1][i]; idles += part[3][i];
            longest = part[2][i] > longest ? part[2][i] : longest;
        }
        feat[(long)b * 4] = cells; feat[(long)b * 4 + 1] = skipped; feat[(long)b * 4 + 2] = longest; feat[(long)b * 4 + 3] = idles;
        const float c0 = rn_div(path_score[b], (float)cells);   // (every integer here is below 2^24: exact as fp32)
        const float c1 = rn_div((float)skipped, (float)Pw);
        const float c2 = rn_div((float)longest, (float)nb);
        const float c3 = rn_div((float)idles, (float)nb);
        total[b] = rn_add(rn_add(rn_add(rn_mul(w0, c0), rn_mul(w1, c1)), rn_mul(w2, c2)), rn_mul(w3, c3));
    }
}

__global__ __launch_bounds__(TK_NT) void take_select_kernel(const float* __restrict__ total, int K, RowCopy x, RowCopy sp, RowCopy ms,
                                                            const int* __restrict__ n_len, int* __restrict__ n_win, int* __restrict__ winner) {
    const int g = blockIdx.y;
    int win = 0;
    float best = total[(long)g * K];
    best = best != best ? INFINITY : best;
    for (int k = 1; k < K; ++k) {   // (uniform: every thread of every workgroup of the group finds the same k)
        float s = total[(long)g * K + k];
        s = s != s ? INFINITY : s;
        if (s < best) { best = s; win = k; }
    }
    const long srow = (long)g * K + win;
    row_copy(x, srow, g, TK_NT);
    row_copy(sp, srow, g, TK_NT);
    row_copy(ms, srow, g, TK_NT);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        n_win[g] = n_len[srow];
        winner[g] = win;
    }
}

}  // namespace

hipError_t launch_take_scores(const float* mass, const int* spans, const float* path_score, const int* n_len, const int* p0, const int* p1,
                              int B, int N, int P, float tau_tok, float tau_frm, float w0, float w1, float w2, float w3, int* feat,
                              float* total, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (N < 1 || P < 1 || N > TK_MAXN || P > TK_MAXP) return hipErrorInvalidValue;
    ProfScope ps(st, "take_scores", 2.0 * B * N * P, 8.0 * B * N * P);
    hipLaunchKernelGGL(take_scores_kernel, dim3(B), dim3(TK_NT), 0, st, mass, spans, path_score, n_len, p0, p1, N, P, tau_tok, tau_frm, w0,
                       w1, w2, w3, feat, total);
    return hipGetLastError();
}

hipError_t launch_take_select(const float* total, int G, int K, int N, int P, const float* x, const int* n_len, const int* spans,
                              const float* mass, float* x_win, int* n_win, int* spans_win, float* mass_win, int* winner, hipStream_t st) {
    if (G <= 0) return hipSuccess;
    if (K < 1 || K > 16 || N < 1 || P < 1 || N > TK_MAXN || P > TK_MAXP || G > 65535) return hipErrorInvalidValue;
    if ((spans != nullptr) != (spans_win != nullptr) || (mass != nullptr) != (mass_win != nullptr)) return hipErrorInvalidValue;
    const RowCopy cx = make_row_copy(x, x_win, (long)N * 64), cs = make_row_copy(spans, spans_win, (long)P * 2),
                   cm = make_row_copy(mass, mass_win, (long)N * P);
    // lanes of the widest copy, four to a thread
    long units = cx.vec ? cx.n4 / 4 : cx.n4;
    if (cm.src) units = std::max(units, cm.vec ? cm.n4 / 4 : cm.n4);
    const int chunks = (int)std::min<long>(64, std::max<long>(1, (units + 4 * TK_NT - 1) / (4 * TK_NT)));
    const double bytes = 4.0 * G * (cx.n4 + (cs.src ? cs.n4 : 0) + (cm.src ? cm.n4 : 0));
    ProfScope ps(st, "take_select", 0.0, 2.0 * bytes);
    hipLaunchKernelGGL(take_select_kernel, dim3(chunks, G), dim3(TK_NT), 0, st, total, K, cx, cs, cm, n_len, n_win, winner);
    return hipGetLastError();
}
