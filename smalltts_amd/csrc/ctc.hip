// CTC score, greedy transcript and best path of per-frame log-probabilities (DESIGN '8i. CTC score', '8l. Forced alignment'), gfx950.
// No weights.
//
// ctc_score: the forward recursion of F.ctc_loss(blank = 0, reduction = 'none', zero_infinity = False), one workgroup per row, thread =
// extended state s of [blank, l_0, blank, l_1, ..., blank] (S = 2 L + 1 <= 397), alpha double-buffered in LDS, one barrier per time
// step; the trip count is the row's frame count, uniform for the workgroup.  A time step is a few dozen cycles of arithmetic, so its
// emission row (C floats) may not be a dependent global load: the rows travel through an LDS ring of two halves of CTC_CH steps.  While
// the workgroup walks one half, the rows of the next half are already in flight as CTC_CH independent loads per thread (the first C
// threads, coalesced) and are parked in the other half before the last barrier of the chunk.
//     alpha_0[0] = lp_0[blank], alpha_0[1] = lp_0[l_0], -inf elsewhere
//     alpha_t[s] = lse3(alpha_{t-1}[s], alpha_{t-1}[s-1], skip(s) ? alpha_{t-1}[s-2] : -inf) + lp_t[label(s)]
//     skip(s)    = s odd, s >= 3 and label(s) != label(s - 2)
//     nll        = -lse2(alpha_{T-1}[S-1], alpha_{T-1}[S-2])
// lse takes the maximum first and returns -inf when it is -inf (never NaN); a NaN operand gives NaN.  An infeasible row ends with every
// reachable alpha at -inf: nll = +inf.  t_len == 0 or L <= 0: +inf.  Tokens are clamped into [1, C) so that no index leaves the row.
//
// ctc_greedy: per frame the class of the largest log-probability (the lowest class on ties; a NaN is never larger), runs collapsed,
// blanks dropped; one workgroup per row, wave = frame for the argmax, then a prefix scan of the keep flags over the row.
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int CTC_NT = 448;        // >= 2 * 198 + 1 extended states, 7 waves
constexpr int CTC_MAXP = 198, CTC_MAXC = 256;
constexpr int CTC_CH = 8;          // steps per ring half = loads in flight per thread

__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);   // (fmaxf drops a NaN operand: the sum below brings it back)
    if (m == -INFINITY && a == a && b == b && c == c) return -INFINITY;
    const float mm = m == -INFINITY ? 0.f : m;
    return mm + logf(expf(a - mm) + expf(b - mm) + expf(c - mm));
}

__global__ __launch_bounds__(CTC_NT) void ctc_score_kernel(const float* __restrict__ logp, const int* __restrict__ t_len,
                                                           const int* __restrict__ tokens, const int* __restrict__ p0a,
                                                           const int* __restrict__ p1a, int T, int P, int C, float* __restrict__ nll) {
    __shared__ float ring[2][CTC_CH][CTC_MAXC];
    __shared__ float alpha[2][CTC_NT];
    const int b = blockIdx.x, s = threadIdx.x;
    int tb = t_len[b], p0 = p0a[b], p1 = p1a[b];
    tb = tb < 0 ? 0 : tb > T ? T : tb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int L = p1 - p0, S = 2 * L + 1;
    if (tb == 0 || L <= 0) {   // (uniform)
        if (s == 0) nll[b] = INFINITY;
        return;
    }
    int lab = 0, lab2 = 0;
    if (s < S && (s & 1)) {
        lab = tokens[(long)b * P + p0 + (s >> 1)];
        lab = lab < 1 ? 1 : lab > C - 1 ? C - 1 : lab;
        if (s >= 3) {
            lab2 = tokens[(long)b * P + p0 + (s >> 1) - 1];
            lab2 = lab2 < 1 ? 1 : lab2 > C - 1 ? C - 1 : lab2;
        }
    }
    const bool skip = (s & 1) && s >= 3 && lab != lab2;
    const float* const lrow = logp + (long)b * T * C;
    const bool loader = s < C;
    // chunk 0 straight into half 0
    if (loader)
        for (int i = 0; i < CTC_CH; ++i) ring[0][i][s] = i < tb ? lrow[(long)i * C + s] : 0.f;
    __syncthreads();
    const int nch = (tb + CTC_CH - 1) / CTC_CH;
    for (int ch = 0; ch < nch; ++ch) {
        const int half = ch & 1, t0 = ch * CTC_CH;
        float nxt[CTC_CH];
        if (loader) {   // the next chunk's rows: CTC_CH loads in flight across this chunk's steps
#pragma unroll
            for (int i = 0; i < CTC_CH; ++i) {
                const int t = t0 + CTC_CH + i;
                nxt[i] = t < tb ? lrow[(long)t * C + s] : 0.f;
            }
        }
        const int nst = tb - t0 < CTC_CH ? tb - t0 : CTC_CH;
        for (int i = 0; i < nst; ++i) {
            const int t = t0 + i;
            const float* const prev = alpha[(t + 1) & 1];
            float* const cur = alpha[t & 1];
            if (s < S) {
                const float lp = ring[half][i][lab];
                float v;
                if (t == 0) {
                    v = s < 2 ? lp : -INFINITY;
                } else {
                    const float a = prev[s];
                    const float bb = s >= 1 ? prev[s - 1] : -INFINITY;
                    const float c = skip ? prev[s - 2] : -INFINITY;
                    v = lse3(a, bb, c) + lp;
                }
                cur[s] = v;
            }
            if (i == nst - 1 && loader) {   // (uniform in i) the other half was last read in the previous chunk, behind a barrier
#pragma unroll
                for (int j = 0; j < CTC_CH; ++j) ring[half ^ 1][j][s] = nxt[j];
            }
            __syncthreads();
        }
    }
    if (s == 0) {
        const float* const fin = alpha[(tb - 1) & 1];
        nll[b] = -lse3(fin[S - 1], fin[S - 2], -INFINITY);
    }
}

// ctc_align: the best path of the same lattice (DESIGN '8l. Forced alignment').  The forward pass is ctc_score's with max in place of
// lse3: no exp / log, one barrier per step, the same ring.  Every thread keeps the 2-bit move of its own state for 16 steps in one
// register and stores one word per 16 steps into the LDS table moves[ceil(tb / 16)][S]; the backtrace of up to 1024 dependent steps then
// reads LDS only (a table in HBM would make it a chain of dependent global loads).  All LDS is one dynamic array sized by the call:
//     ring 2 * CTC_CH * CTC_MAXC floats | delta 2 * CTC_NT floats | first / last 2 * CTC_MAXP ints | state T u16 | moves ceil(T / 16) * (2 P + 1) words
// 125 248 bytes at T = 1024, P = 198 (the move table 101 632 of them): raised past the 64 KB default as attention_img.hip does.
// Definition and output contract: include/smalltts_hip.h (smtts_ctc_align).
constexpr int AL_MAXT = 1024;
constexpr size_t AL_OFF_DELTA = sizeof(float) * 2 * CTC_CH * CTC_MAXC;           // 16384
constexpr size_t AL_OFF_FL = AL_OFF_DELTA + sizeof(float) * 2 * CTC_NT;          // + 3584
constexpr size_t AL_OFF_STATE = AL_OFF_FL + sizeof(int) * 2 * 200;               // + 1600 (CTC_MAXP rounded up to keep 16-byte offsets)
static inline size_t al_off_moves(int T) { return AL_OFF_STATE + (((size_t)T * 2 + 15) & ~(size_t)15); }
static inline size_t al_lds_bytes(int T, int P) { return al_off_moves(T) + (size_t)((T + 15) / 16) * (2 * P + 1) * 4; }

__global__ __launch_bounds__(CTC_NT) void ctc_align_kernel(const float* __restrict__ logp, const int* __restrict__ t_len,
                                                           const int* __restrict__ tokens, const int* __restrict__ p0a,
                                                           const int* __restrict__ p1a, int T, int P, int C, int off_moves,
                                                           int* __restrict__ spans, float* __restrict__ tok_logp,
                                                           int* __restrict__ frame_tok, float* __restrict__ score) {
    extern __shared__ __attribute__((aligned(16))) char al_smem[];
    float (*const ring)[CTC_CH][CTC_MAXC] = reinterpret_cast<float (*)[CTC_CH][CTC_MAXC]>(al_smem);
    float (*const delta)[CTC_NT] = reinterpret_cast<float (*)[CTC_NT]>(al_smem + AL_OFF_DELTA);
    int* const first = reinterpret_cast<int*>(al_smem + AL_OFF_FL);
    int* const last = first + 200;
    unsigned short* const state = reinterpret_cast<unsigned short*>(al_smem + AL_OFF_STATE);
    unsigned* const moves = reinterpret_cast<unsigned*>(al_smem + off_moves);
    const int b = blockIdx.x, s = threadIdx.x;
    int tb = t_len[b], p0 = p0a[b], p1 = p1a[b];
    tb = tb < 0 ? 0 : tb > T ? T : tb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int L = p1 - p0, S = 2 * L + 1, SW = 2 * P + 1;
    int* const sp = spans + (long)b * P * 2;
    float* const tl = tok_logp + (long)b * P;
    int* const ft = frame_tok ? frame_tok + (long)b * T : nullptr;
    const float* const lrow = logp + (long)b * T * C;
    bool aligned = false;
    int lab = 0;
    if (tb == 0 || L <= 0) {   // (uniform)
        if (s == 0) score[b] = -INFINITY;
    } else {
        int lab2 = 0;
        if (s < S && (s & 1)) {
            lab = tokens[(long)b * P + p0 + (s >> 1)];
            lab = lab < 1 ? 1 : lab > C - 1 ? C - 1 : lab;
            if (s >= 3) {
                lab2 = tokens[(long)b * P + p0 + (s >> 1) - 1];
                lab2 = lab2 < 1 ? 1 : lab2 > C - 1 ? C - 1 : lab2;
            }
        }
        const bool skip = (s & 1) && s >= 3 && lab != lab2;
        const bool loader = s < C;
        if (loader)
            for (int i = 0; i < CTC_CH; ++i) ring[0][i][s] = i < tb ? lrow[(long)i * C + s] : 0.f;
        __syncthreads();
        const int nch = (tb + CTC_CH - 1) / CTC_CH;
        unsigned mv = 0;   // this state's moves of the current 16 steps, step t at bits 2 (t & 15)
        for (int ch = 0; ch < nch; ++ch) {
            const int half = ch & 1, t0 = ch * CTC_CH;
            float nxt[CTC_CH];
            if (loader) {   // the next chunk's rows: CTC_CH loads in flight across this chunk's steps
#pragma unroll
                for (int i = 0; i < CTC_CH; ++i) {
                    const int t = t0 + CTC_CH + i;
                    nxt[i] = t < tb ? lrow[(long)t * C + s] : 0.f;
                }
            }
            const int nst = tb - t0 < CTC_CH ? tb - t0 : CTC_CH;
            for (int i = 0; i < nst; ++i) {
                const int t = t0 + i;
                const float* const prev = delta[(t + 1) & 1];
                float* const cur = delta[t & 1];
                if (s < S) {
                    const float lp = ring[half][i][lab];
                    float v;
                    if (t == 0) {
                        v = s < 2 ? lp : -INFINITY;
                    } else {
                        v = prev[s];
                        unsigned m = 0;
                        if (s >= 1) {
                            const float a = prev[s - 1];
                            if (a > v) { v = a; m = 1; }
                        }
                        if (skip) {
                            const float a = prev[s - 2];
                            if (a > v) { v = a; m = 2; }
                        }
                        v = v + lp;
                        mv |= m << (2 * (t & 15));
                    }
                    cur[s] = v;
                    if ((t & 15) == 15 || t == tb - 1) {   // (uniform in t)
                        moves[(t >> 4) * SW + s] = mv;
                        mv = 0;
                    }
                }
                if (i == nst - 1 && loader) {   // (uniform in i) the other half was last read in the previous chunk, behind a barrier
#pragma unroll
                    for (int j = 0; j < CTC_CH; ++j) ring[half ^ 1][j][s] = nxt[j];
                }
                __syncthreads();
            }
        }
        const float* const fin = delta[(tb - 1) & 1];
        const int e = fin[S - 2] > fin[S - 1] ? S - 2 : S - 1;
        const float sc = fin[e];
        aligned = sc > -INFINITY;   // (uniform; false for NaN)
        if (s == 0) {
            score[b] = sc;
            if (aligned) {   // tb - 1 dependent LDS reads; the index stays inside [0, S) whatever the table holds
                int q = e;
                for (int t = tb - 1; t >= 1; --t) {
                    state[t] = (unsigned short)q;
                    const unsigned m = (moves[(t >> 4) * SW + q] >> (2 * (t & 15))) & 3u;
                    q -= (int)m;
                    q = q < 0 ? 0 : q;
                }
                state[0] = (unsigned short)q;
            }
        }
    }
    if (s < 200) { first[s] = -1; last[s] = -1; }
    __syncthreads();
    if (aligned) {   // thread = frame: the ends of every label state's run (states never decrease along t: one run, one writer each)
        for (int t = s; t < tb; t += CTC_NT) {
            const int q = state[t];
            if (q & 1) {
                if (t == 0 || state[t - 1] != q) first[q >> 1] = t;
                if (t == tb - 1 || state[t + 1] != q) last[q >> 1] = t;
            }
        }
    }
    __syncthreads();
    if (s < P) {   // thread = token
        const int j = s - p0;
        const int f = aligned && j >= 0 && j < L ? first[j] : -1, l = f >= 0 ? last[j] : -1;
        float acc = 0.f;
        if (f >= 0) {   // t ascending, single adds
            int c = tokens[(long)b * P + s];
            c = c < 1 ? 1 : c > C - 1 ? C - 1 : c;
            for (int t = f; t <= l; ++t) acc += lrow[(long)t * C + c];
        }
        sp[2 * s] = f;
        sp[2 * s + 1] = l;
        tl[s] = acc;
    }
    if (ft)
        for (int t = s; t < T; t += CTC_NT) {
            int v = -1;
            if (aligned && t < tb) {
                const int q = state[t];
                if (q & 1) v = p0 + (q >> 1);
            }
            ft[t] = v;
        }
}

constexpr int GR_NT = 256, GR_MAXT = 4096;

__global__ __launch_bounds__(GR_NT) void ctc_greedy_kernel(const float* __restrict__ logp, const int* __restrict__ t_len, int T, int C,
                                                           int* __restrict__ ids, int* __restrict__ n_ids) {
    __shared__ int am[GR_MAXT];
    __shared__ int cnt[GR_NT];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int tb = t_len[b];
    tb = tb < 0 ? 0 : tb > T ? T : tb;
    const float* const lrow = logp + (long)b * T * C;
    for (int f = w; f < tb; f += GR_NT / 64) {
        float best = -INFINITY;
        int bi = C;   // "none yet": any class beats it on a tie
        for (int c = lane; c < C; c += 64) {
            const float v = lrow[(long)f * C + c];
            if (v > best || (v == best && c < bi)) { best = v; bi = c; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) am[f] = bi >= C ? 0 : bi;   // a frame of NaNs: blank
    }
    __syncthreads();
    // thread tid owns the frames [f0, f1); keep = not blank and not the class of the frame before
    const int per = (tb + GR_NT - 1) / GR_NT;
    const int f0 = tid * per < tb ? tid * per : tb, f1 = f0 + per < tb ? f0 + per : tb;
    int n = 0;
    for (int f = f0; f < f1; ++f) n += am[f] != 0 && (f == 0 || am[f] != am[f - 1]);
    cnt[tid] = n;
    __syncthreads();
    for (int o = 1; o < GR_NT; o <<= 1) {   // inclusive scan
        const int v = tid >= o ? cnt[tid - o] : 0;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    const int total = cnt[GR_NT - 1];
    int at = cnt[tid] - n;
    int* const out = ids + (long)b * T;
    for (int f = f0; f < f1; ++f)
        if (am[f] != 0 && (f == 0 || am[f] != am[f - 1])) out[at++] = am[f];
    for (int i = total + tid; i < T; i += GR_NT) out[i] = 0;
    if (tid == 0) n_ids[b] = total;
}

}  // namespace

hipError_t launch_ctc_score(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P, int C,
                            float* nll, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (T < 1 || P < 1 || P > CTC_MAXP || C < 2 || C > CTC_MAXC) return hipErrorInvalidValue;
    ProfScope ps(st, "ctc_score", 12.0 * B * T * (2.0 * P + 1), 4.0 * B * T * C);
    hipLaunchKernelGGL(ctc_score_kernel, dim3(B), dim3(CTC_NT), 0, st, logp, t_len, tokens, p0, p1, T, P, C, nll);
    return hipGetLastError();
}

hipError_t launch_ctc_align(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P, int C,
                            int* spans, float* tok_logp, int* frame_tok, float* score, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (T < 1 || T > AL_MAXT || P < 1 || P > CTC_MAXP || C < 2 || C > CTC_MAXC) return hipErrorInvalidValue;
    static DevOnce once;
    hipError_t e = once.ensure([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)al_lds_bytes(AL_MAXT, CTC_MAXP));
    });
    if (e != hipSuccess) return e;
    ProfScope ps(st, "ctc_align", 6.0 * B * T * (2.0 * P + 1), 4.0 * B * T * C);
    hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(CTC_NT), al_lds_bytes(T, P), st, logp, t_len, tokens, p0, p1, T, P, C,
                       (int)al_off_moves(T), spans, tok_logp, frame_tok, score);
    return hipGetLastError();
}

hipError_t launch_ctc_greedy(const float* logp, const int* t_len, int B, int T, int C, int* ids, int* n_ids, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (T < 1 || T > GR_MAXT || C < 1) return hipErrorInvalidValue;
    ProfScope ps(st, "ctc_greedy", 2.0 * B * T * C, 4.0 * B * T * C);
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(GR_NT), 0, st, logp, t_len, T, C, ids, n_ids);
    return hipGetLastError();
}
