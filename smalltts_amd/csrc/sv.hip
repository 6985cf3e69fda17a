// The latent speaker verifier (DESIGN '8j. Speaker score'): 64-dim latents -> one 192-dim speaker embedding per row, gfx950.
//   ECAPA-TDNN: TDNN(64 -> 768, k 3) -> three SERes2Net blocks at width 768 (dilations 2, 3, 5: TDNN k 1, an 11-band Res2Net chain of
//   TDNN(64 -> 64, k 3, d), TDNN k 1, squeeze-excite gate, residual) -> TDNN(2304 -> 2304) on the three block outputs -> attentive
//   statistics pooling -> BatchNorm -> 4608 -> 192.  A TDNN is conv, ReLU, BatchNorm (eval, folded to scale / shift at finalize).
// fp32 operands and fp32 accumulation throughout: every wide product runs on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32, a k-ordered
// fmaf chain), the per-row vectors on plain FMA chains.  Every row of the batch is computed as if it were alone at its own length n_b:
// reflect padding reflects about the row's own first and last frame, every mean / softmax / statistic runs over [0, n_b), nothing at or
// behind n_b is read, and every tile starts at the row's frame 0, so that a row's sums have one order whatever the batch.  A row with
// n_b < 6 (the d = 5 reflect needs pad < n) has no embedding: its emb row is 0.0 and no other kernel touches it.
//   sv_tdnn       64 frames x 64 outputs per workgroup, wave w owns one 32 x 32 block; the K dimension streams through LDS in blocks
//                 of 64 (activations transposed [k][frame] with the bank permutation of f32_tile.hpp, the weight block [k][n] as packed at
//                 finalize), the next block's global loads in flight under the current block's products.  K blocks come from up to
//                 three source tensors (mfa: the concatenation is never materialised) or from three taps of one (blocks.0: reflect
//                 indexing on load).  Epilogues: bias; ReLU + affine; row constant + ReLU + affine + tanh (the pooling's attention).
//   sv_res2net    one workgroup per row: the running band u_i = x_i + y_{i-1} of the whole row sits in LDS [channel][frame], next to
//                 the band's 192 x 64 weights; bands are walked in order, one barrier pair per band, the reflect index computed per tap.
//                 Kept over eleven tiled launches per block (band i reading band i - 1 from memory): 185 us against 261 us per block
//                 at 32 rows x 75 frames, the same bits.
//   sv_se_squeeze one workgroup per row: time mean in frame order, 768 -> 192 -> 768, sigmoid -> gate (B, 768)
//   sv_se_apply   gate * x + r
//   sv_asp_stats  uniform mean and two-pass std per row and channel;  sv_rowvec: 4608 -> 192 per row (the pooling's row constant
//                 c = W[:, 2304:] [m ; s], and the final fc), four k segments of fixed extent summed in order
//   sv_asp_pool   per row and channel: softmax over the row's frames (maximum first, expf), weighted mean, two-pass std, asp_bn affine
//   sv_cosine     one wave per row, a fixed butterfly
// No atomics.  Workspace contents are irrelevant: every buffer element that is read was written by an earlier kernel of the same call.
#include "f32_tile.hpp"
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int S_NT = 256, S_TM = 64, S_LD = 64;
constexpr int S_C = 768, S_BAND = 64, S_NBAND = 12, S_SE = 192, S_ATT = 192, S_MFA = 2304, S_POOL = 4608, S_EMB = 192, S_IN = 64;
constexpr int S_MIN = 6, S_MAXN = 225;
constexpr float S_ASP_EPS = 1e-12f;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// index t (|t - [0, n)| < n) reflected about the row's first and last frame
__device__ __forceinline__ int reflect(int t, int n) { return t < 0 ? -t : t >= n ? 2 * (n - 1) - t : t; }

// MODE 0: acc + b;  1: scale * relu(acc + b) + shift;  2: tanh(scale * relu(acc + b + c[row]) + shift)
template <int MODE>
__global__ __launch_bounds__(S_NT) void sv_tdnn_kernel(const float* __restrict__ s0, const float* __restrict__ s1,
                                                       const float* __restrict__ s2, int cin /* channels of a source frame */,
                                                       int kps /* K blocks per source (or per tap) */, int taps, int dil, int nkb,
                                                       const int* __restrict__ n_len, int N, SvTdnnW w,
                                                       const float* __restrict__ crow, float* __restrict__ y, int cout) {
    __shared__ __attribute__((aligned(16))) float aT[S_TM * S_LD], wS[S_LD * S_LD];
    const int b = blockIdx.z, ob = blockIdx.y, t0 = blockIdx.x * S_TM, n = row_len(n_len, b, N);
    if (n < S_MIN || t0 >= n) return;   // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f0 = 32 * (wv >> 1), n0 = 32 * (wv & 1), col = n0 + (lane & 31), rbase = f0 + 4 * (lane >> 5);
    const f32x4* const wbase = reinterpret_cast<const f32x4*>(w.wt + (long)ob * nkb * (S_LD * S_LD));
    float av[16];
    f32x4 wr[4];
#define SV_FETCH(kb_)                                                                                                        \
    {                                                                                                                        \
        const int kq = (kb_), s = kq / kps, c0 = (kq - s * kps) * 64;                                                        \
        const float* const src = (taps == 3 || s == 0) ? s0 : s == 1 ? s1 : s2;                                              \
        const int off = taps == 3 ? (s - 1) * dil : 0;                                                                       \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                                                     \
            const int t = t0 + wv + 4 * i; /* (uniform per wave) */                                                          \
            av[i] = t < n ? src[((long)b * N + reflect(t + off, n)) * cin + c0 + lane] : 0.f;                                \
        }                                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) wr[i] = wbase[(long)kq * (S_LD * S_LD / 4) + tid + S_NT * i];          \
    }
#define SV_PUT()                                                                                                             \
    {                                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) aT[tile_at<S_LD>(lane, wv + 4 * i)] = av[i];                                   \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) reinterpret_cast<f32x4*>(wS)[tid + S_NT * i] = wr[i];                  \
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    SV_FETCH(0)
    SV_PUT()
    __syncthreads();
    const int r = lane & 31, h = lane >> 5;
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb + 1 < nkb) SV_FETCH(kb + 1)
#pragma unroll 8
        for (int k = 0; k < S_LD; k += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aT[tile_at<S_LD>(k + h, f0 + r)], wS[(k + h) * S_LD + n0 + r], acc, 0, 0, 0);
        __syncthreads();
        if (kb + 1 < nkb) SV_PUT()
        __syncthreads();
    }
    const int o = ob * 64 + col;
    const float bias = w.b[o] + (MODE == 2 ? crow[(long)b * cout + o] : 0.f);
    const float sc = MODE ? w.scale[o] : 1.f, sh = MODE ? w.shift[o] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = t0 + rbase + (i & 3) + 8 * (i >> 2);
        if (t >= n) continue;
        float v = acc[i] + bias;
        if (MODE) v = fmaf(fmaxf(v, 0.f), sc, sh);
        if (MODE == 2) v = tanhf(v);
        y[((long)b * N + t) * cout + o] = v;
    }
#undef SV_FETCH
#undef SV_PUT
}

// ---- Res2Net chain: one workgroup per row ----------------------------------------------------------------------------------------------
constexpr int R_NT = 512, R_LD = 256 /* >= 225 frames, a multiple of 64 */, R_K = 3 * S_BAND;
constexpr size_t R_LDS = (size_t)(S_BAND * R_LD + R_K * S_BAND) * 4;   // 64 KB running band + 48 KB weights
__device__ __forceinline__ int r_at(int k, int f) { return k * R_LD + (f & ~63) + 4 * (((f & 63) >> 2) ^ (k & 15)) + (f & 3); }

__global__ __launch_bounds__(R_NT) void sv_res2net_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const int* __restrict__ n_len, int N, SvBlockW w) {
    extern __shared__ __attribute__((aligned(16))) float sv_lds[];
    float* const uT = sv_lds;                    // [64 channels][R_LD frames] (r_at)
    float* const wS = sv_lds + S_BAND * R_LD;    // [192 k = tap * 64 + channel][64 outputs]
    const int b = blockIdx.x, n = row_len(n_len, b, N);
    if (n < S_MIN) return;   // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, d = w.dil;
    const float* const xr = x + (long)b * N * S_C;
    float* const yr = y + (long)b * N * S_C;
    for (int f = wv; f < n; f += R_NT / 64) {   // band 0 passes through; band 1's input is x_1
        yr[(long)f * S_C + lane] = xr[(long)f * S_C + lane];
        uT[r_at(lane, f)] = xr[(long)f * S_C + S_BAND + lane];
    }
    const int nblk = 2 * ((n + 31) / 32);   // 32 x 32 blocks of the row: at most 16, two per wave
    const int r = lane & 31, h = lane >> 5;
    for (int band = 1; band < S_NBAND; ++band) {
        const SvTdnnW tw = w.band[band - 1];
        for (int i = tid; i < R_K * S_BAND / 4; i += R_NT)
            reinterpret_cast<float4*>(wS)[i] = reinterpret_cast<const float4*>(tw.wt)[i];
        __syncthreads();   // weights and the running band are in place
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
            const int blk = wv + (R_NT / 64) * j;
            if (blk >= nblk) continue;   // (uniform per wave)
            const int f0 = 32 * (blk >> 1), n0 = 32 * (blk & 1);
            const int fc = min(f0 + r, n - 1);   // lanes behind the row's end repeat its last frame; their results are dropped
#pragma unroll
            for (int tap = 0; tap < 3; ++tap) {
                const int ft = reflect(fc + (tap - 1) * d, n);
#pragma unroll 8
                for (int k = 0; k < S_BAND; k += 2)
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(uT[r_at(k + h, ft)], wS[(tap * S_BAND + k + h) * S_BAND + n0 + r],
                                                                  acc[j], 0, 0, 0);
            }
        }
        __syncthreads();   // every read of the running band and of the weights is done
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int blk = wv + (R_NT / 64) * j;
            if (blk >= nblk) continue;
            const int f0 = 32 * (blk >> 1), col = 32 * (blk & 1) + r;
            const float bias = tw.b[col], sc = tw.scale[col], sh = tw.shift[col];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int f = f0 + 4 * h + (i & 3) + 8 * (i >> 2);
                if (f >= n) continue;
                const float v = fmaf(fmaxf(acc[j][i] + bias, 0.f), sc, sh);
                yr[(long)f * S_C + band * S_BAND + col] = v;
                if (band + 1 < S_NBAND) uT[r_at(col, f)] = xr[(long)f * S_C + (band + 1) * S_BAND + col] + v;
            }
        }
    }
}

// ---- squeeze-excite --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(S_C) void sv_se_squeeze_kernel(const float* __restrict__ x, const int* __restrict__ n_len, int N,
                                                            SvBlockW w, float* __restrict__ gate) {
    __shared__ float sm[S_C], hs[S_SE];
    const int b = blockIdx.x, n = row_len(n_len, b, N), c = threadIdx.x;
    if (n < S_MIN) return;
    const float* const xr = x + (long)b * N * S_C + c;
    float s = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) s += xr[(long)f * S_C];
    sm[c] = s / (float)n;
    __syncthreads();
    if (c < S_SE) {
        float a = w.se_b1[c];
#pragma unroll 8
        for (int k = 0; k < S_C; ++k) a = fmaf(w.se_w1t[k * S_SE + c], sm[k], a);
        hs[c] = fmaxf(a, 0.f);
    }
    __syncthreads();
    float g = w.se_b2[c];
#pragma unroll 8
    for (int k = 0; k < S_SE; ++k) g = fmaf(w.se_w2t[k * S_C + c], hs[k], g);
    gate[(long)b * S_C + c] = 1.0f / (1.0f + expf(-g));
}

__global__ __launch_bounds__(S_NT) void sv_se_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           const float* __restrict__ gate, const int* __restrict__ n_len, int N,
                                                           float* __restrict__ y) {
    const int b = blockIdx.y, n = row_len(n_len, b, N);
    const int i = blockIdx.x * S_NT + threadIdx.x, f = i / (S_C / 4), c4 = i - f * (S_C / 4);
    if (n < S_MIN || f >= n) return;
    const long at = ((long)b * N + f) * (S_C / 4) + c4;
    const float4 xv = reinterpret_cast<const float4*>(x)[at], rv = reinterpret_cast<const float4*>(res)[at];
    const float4 g = reinterpret_cast<const float4*>(gate)[(long)b * (S_C / 4) + c4];
    reinterpret_cast<float4*>(y)[at] = make_float4(g.x * xv.x + rv.x, g.y * xv.y + rv.y, g.z * xv.z + rv.z, g.w * xv.w + rv.w);
}

// ---- attentive statistics pooling -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(S_NT) void sv_asp_stats_kernel(const float* __restrict__ x, const int* __restrict__ n_len, int N,
                                                            float* __restrict__ ms) {
    const int b = blockIdx.y, n = row_len(n_len, b, N), c = blockIdx.x * S_NT + threadIdx.x;
    if (n < S_MIN) return;
    const float* const xr = x + (long)b * N * S_MFA + c;
    const float wgt = 1.0f / (float)n;
    float m = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) m = fmaf(wgt, xr[(long)f * S_MFA], m);
    float v = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) {
        const float dv = xr[(long)f * S_MFA] - m;
        v = fmaf(wgt, dv * dv, v);
    }
    ms[(long)b * S_POOL + c] = m;
    ms[(long)b * S_POOL + S_MFA + c] = sqrtf(fmaxf(v, S_ASP_EPS));
}

// out[b][o] = bias[o] + sum_k W[o][k] v[b][k], K = 4608, 192 outputs: thread (segment, o) sums its quarter of k in order, the four
// partial sums are added in segment order.  A row with n_b < 6: 0.0 where zero_short, untouched otherwise.
constexpr int V_SEG = 4, V_NT = V_SEG * S_EMB;
__global__ __launch_bounds__(V_NT) void sv_rowvec_kernel(const float* __restrict__ v, const float* __restrict__ wt /* [4608][192] */,
                                                         const float* __restrict__ bias /* or NULL */, const int* __restrict__ n_len,
                                                         int N, int zero_short, float* __restrict__ out) {
    __shared__ float vs[S_POOL], part[V_SEG][S_EMB];
    const int b = blockIdx.x, n = row_len(n_len, b, N), tid = threadIdx.x, seg = tid / S_EMB, o = tid - seg * S_EMB;
    if (n < S_MIN) {   // (uniform)
        if (zero_short && tid < S_EMB) out[(long)b * S_EMB + tid] = 0.f;
        return;
    }
    for (int i = tid; i < S_POOL; i += V_NT) vs[i] = v[(long)b * S_POOL + i];
    __syncthreads();
    constexpr int KS = S_POOL / V_SEG;
    float a = 0.f;
#pragma unroll 8
    for (int k = seg * KS; k < (seg + 1) * KS; ++k) a = fmaf(wt[(long)k * S_EMB + o], vs[k], a);
    part[seg][o] = a;
    __syncthreads();
    if (seg == 0) out[(long)b * S_EMB + o] = (((part[0][o] + part[1][o]) + part[2][o]) + part[3][o]) + (bias ? bias[o] : 0.f);
}

__global__ __launch_bounds__(S_NT) void sv_asp_pool_kernel(const float* __restrict__ lg, const float* __restrict__ x,
                                                           const int* __restrict__ n_len, int N, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float* __restrict__ pooled) {
    const int b = blockIdx.y, n = row_len(n_len, b, N), c = blockIdx.x * S_NT + threadIdx.x;
    if (n < S_MIN) return;
    const float* const lr = lg + (long)b * N * S_MFA + c;
    const float* const xr = x + (long)b * N * S_MFA + c;
    float mx = -INFINITY;
#pragma unroll 8
    for (int f = 0; f < n; ++f) mx = fmaxf(mx, lr[(long)f * S_MFA]);
    float l = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) l += expf(lr[(long)f * S_MFA] - mx);
    const float inv = 1.0f / l;
    float m = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) m = fmaf(expf(lr[(long)f * S_MFA] - mx) * inv, xr[(long)f * S_MFA], m);
    float v = 0.f;
#pragma unroll 8
    for (int f = 0; f < n; ++f) {
        const float dv = xr[(long)f * S_MFA] - m;
        v = fmaf(expf(lr[(long)f * S_MFA] - mx) * inv, dv * dv, v);
    }
    pooled[(long)b * S_POOL + c] = fmaf(m, scale[c], shift[c]);
    pooled[(long)b * S_POOL + S_MFA + c] = fmaf(sqrtf(fmaxf(v, S_ASP_EPS)), scale[S_MFA + c], shift[S_MFA + c]);
}

// ---- cosine: row b of emb against row b / K of ref; one wave per row ----------------------------------------------------------------
__global__ __launch_bounds__(S_NT) void sv_cosine_kernel(const float* __restrict__ emb, const float* __restrict__ ref, int B, int K,
                                                         int D, float* __restrict__ out) {
    const int b = blockIdx.x * (S_NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;   // (uniform per wave)
    const float* const a = emb + (long)b * D;
    const float* const r = ref + (long)(b / K) * D;
    float ar = 0.f, aa = 0.f, rr = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float av = a[i], rv = r[i];
        ar = fmaf(av, rv, ar); aa = fmaf(av, av, aa); rr = fmaf(rv, rv, rr);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {   // (a + b == b + a: every lane ends with the same bits)
        ar += __shfl_xor(ar, o, 64); aa += __shfl_xor(aa, o, 64); rr += __shfl_xor(rr, o, 64);
    }
    if (lane == 0) out[b] = ar / (fmaxf(sqrtf(aa), 1e-8f) * fmaxf(sqrtf(rr), 1e-8f));
}

DevOnce g_sv_once;

template <int MODE>
void tdnn(hipStream_t st, const char* name, const float* s0, const float* s1, const float* s2, int cin, int kps, int taps, int dil, int K,
          const int* n_len, int B, int N, const SvTdnnW& w, const float* crow, float* y, int cout) {
    const double fr = (double)B * N;
    ProfScope ps(st, name, 2.0 * fr * K * cout, 4.0 * fr * (K + cout) + 4.0 * K * cout);
    hipLaunchKernelGGL((sv_tdnn_kernel<MODE>), dim3((N + S_TM - 1) / S_TM, cout / 64, B), dim3(S_NT), 0, st, s0, s1, s2, cin, kps, taps,
                       dil, K / 64, n_len, N, w, crow, y, cout);
}

}  // namespace

// per frame: blocks.0 / tdnn (aliased by tdnn2) / res2net, then the three block outputs, mfa, attention; the 2304 logits alias the first
// three; per row: gate, [m ; s], the row constant, pooled
size_t sv_ws_bytes(int B, int N) {
    const size_t fr = (size_t)B * N;
    return 6 * up256(fr * S_C * 4) + up256(fr * S_MFA * 4) + up256(fr * S_ATT * 4) + up256((size_t)B * S_C * 4) +
           2 * up256((size_t)B * S_POOL * 4) + up256((size_t)B * S_ATT * 4);
}

// launch order: blocks.0; per block tdnn1, res2net, tdnn2, se_squeeze, se_apply; mfa, stats, row constant, attention, logits, pool, fc
size_t sv_tap_bytes(int B, int N, int slot) {
    if (slot < 0 || slot >= SV_TAPS) return 0;
    const size_t fr = (size_t)B * N;
    if (slot < 16) return slot && (slot - 1) % 5 == 3 ? (size_t)B * S_C * 4 : fr * S_C * 4;
    static const int per_frame[7] = {S_MFA, 0, 0, S_ATT, S_MFA, 0, 0}, per_row[7] = {0, S_POOL, S_ATT, 0, 0, S_POOL, S_EMB};
    return (fr * per_frame[slot - 16] + (size_t)B * per_row[slot - 16]) * 4;
}

hipError_t launch_sv_embed(const SvW& w, const float* x, const int* n_len, int B, int N, void* ws, float* emb, hipStream_t st,
                           const ScorerTaps* taps) {
    if (B < 1 || N < S_MIN || N > S_MAXN) return hipErrorInvalidValue;
    hipError_t e = g_sv_once.ensure([] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(sv_res2net_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)R_LDS);
    });
    if (e != hipSuccess) return e;
    const size_t fr = (size_t)B * N;
    char* p = static_cast<char*>(ws);
    auto take = [&](size_t bytes) { float* q = reinterpret_cast<float*>(p); p += up256(bytes); return q; };
    float* const h0 = take(fr * S_C * 4);   // (h0, t1, r2 are consecutive: up256 of a multiple of 256 bytes adds nothing)
    float* const t1 = take(fr * S_C * 4);
    float* const r2 = take(fr * S_C * 4);
    float* const ob[3] = {take(fr * S_C * 4), take(fr * S_C * 4), take(fr * S_C * 4)};
    float* const mfa = take(fr * S_MFA * 4);
    float* const att = take(fr * S_ATT * 4);
    float* const gate = take((size_t)B * S_C * 4);
    float* const ms = take((size_t)B * S_POOL * 4);
    float* const pooled = take((size_t)B * S_POOL * 4);
    float* const crow = take((size_t)B * S_ATT * 4);
    float* const logit = h0;   // fr * 2304 floats = h0 + t1 + r2, all dead once mfa is written
    const double frd = (double)fr;
    int slot = 0;
    hipError_t te = hipSuccess;
    auto tap = [&](const float* buf) {   // (tests only) what the launch just enqueued wrote, into its slot
        if (!taps) return;
        const hipError_t e = hipMemcpyAsync(taps->base + taps->off[slot], buf, sv_tap_bytes(B, N, slot), hipMemcpyDeviceToDevice, st);
        if (te == hipSuccess) te = e;
        ++slot;
    };
    tdnn<1>(st, "sv_tdnn", x, nullptr, nullptr, S_IN, 1, 3, 1, 3 * S_IN, n_len, B, N, w.in, nullptr, h0, S_C);
    tap(h0);
    for (int i = 0; i < 3; ++i) {
        const SvBlockW& bw = w.block[i];
        const float* const in = i ? ob[i - 1] : h0;
        tdnn<1>(st, "sv_tdnn", in, nullptr, nullptr, S_C, S_C / 64, 1, 1, S_C, n_len, B, N, bw.tdnn1, nullptr, t1, S_C);
        tap(t1);
        {
            ProfScope ps(st, "sv_res2net", 2.0 * frd * (S_NBAND - 1) * R_K * S_BAND, 8.0 * frd * S_C);
            hipLaunchKernelGGL(sv_res2net_kernel, dim3(B), dim3(R_NT), R_LDS, st, t1, r2, n_len, N, bw);
        }
        tap(r2);
        tdnn<1>(st, "sv_tdnn", r2, nullptr, nullptr, S_C, S_C / 64, 1, 1, S_C, n_len, B, N, bw.tdnn2, nullptr, t1, S_C);
        tap(t1);
        {
            ProfScope ps(st, "sv_se_squeeze", 4.0 * B * S_C * S_SE + frd * S_C, 4.0 * frd * S_C);
            hipLaunchKernelGGL(sv_se_squeeze_kernel, dim3(B), dim3(S_C), 0, st, t1, n_len, N, bw, gate);
        }
        tap(gate);
        {
            ProfScope ps(st, "sv_se_apply", 2.0 * frd * S_C, 12.0 * frd * S_C);
            hipLaunchKernelGGL(sv_se_apply_kernel, dim3((N * (S_C / 4) + S_NT - 1) / S_NT, B), dim3(S_NT), 0, st, t1, in, gate, n_len, N,
                               ob[i]);
        }
        tap(ob[i]);
    }
    tdnn<1>(st, "sv_tdnn", ob[0], ob[1], ob[2], S_C, S_C / 64, 1, 1, S_MFA, n_len, B, N, w.mfa, nullptr, mfa, S_MFA);
    tap(mfa);
    {
        ProfScope ps(st, "sv_asp_stats", 5.0 * frd * S_MFA, 8.0 * frd * S_MFA);
        hipLaunchKernelGGL(sv_asp_stats_kernel, dim3(S_MFA / S_NT, B), dim3(S_NT), 0, st, mfa, n_len, N, ms);
    }
    tap(ms);
    {
        ProfScope ps(st, "sv_asp_const", 2.0 * B * S_POOL * S_ATT, 4.0 * S_POOL * S_ATT);
        hipLaunchKernelGGL(sv_rowvec_kernel, dim3(B), dim3(V_NT), 0, st, ms, w.att_ct, nullptr, n_len, N, 0, crow);
    }
    tap(crow);
    tdnn<2>(st, "sv_tdnn", mfa, nullptr, nullptr, S_MFA, S_MFA / 64, 1, 1, S_MFA, n_len, B, N, w.att, crow, att, S_ATT);
    tap(att);
    tdnn<0>(st, "sv_tdnn", att, nullptr, nullptr, S_ATT, S_ATT / 64, 1, 1, S_ATT, n_len, B, N, w.logit, nullptr, logit, S_MFA);
    tap(logit);
    {
        ProfScope ps(st, "sv_asp_pool", 12.0 * frd * S_MFA, 8.0 * frd * S_MFA);
        hipLaunchKernelGGL(sv_asp_pool_kernel, dim3(S_MFA / S_NT, B), dim3(S_NT), 0, st, logit, mfa, n_len, N, w.pool_scale, w.pool_shift,
                           pooled);
    }
    tap(pooled);
    {
        ProfScope ps(st, "sv_fc", 2.0 * B * S_POOL * S_EMB, 4.0 * S_POOL * S_EMB);
        hipLaunchKernelGGL(sv_rowvec_kernel, dim3(B), dim3(V_NT), 0, st, pooled, w.fc_t, w.fc_b, n_len, N, 1, emb);
    }
    tap(emb);
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : te;
}

hipError_t launch_sv_cosine(const float* emb, const float* ref, int B, int K, int D, float* cos, hipStream_t st) {
    if (B < 1 || K < 1 || B % K || D < 1) return hipErrorInvalidValue;
    ProfScope ps(st, "sv_cosine", 6.0 * B * D, 8.0 * B * D);
    hipLaunchKernelGGL(sv_cosine_kernel, dim3((B + S_NT / 64 - 1) / (S_NT / 64)), dim3(S_NT), 0, st, emb, ref, B, K, D, cos);
    return hipGetLastError();
}
