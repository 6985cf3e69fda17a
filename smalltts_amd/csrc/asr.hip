// The latent phoneme recogniser (DESIGN '8i. CTC score'): 64-dim latents -> per-frame log-probabilities over 198 phoneme classes, gfx950.
//   upsample x4 (depthwise ConvTranspose, kernel = stride = 4) -> 7 Conformer layers at width 64 (half-step FFN, 16-head self-attention,
//   conv module, half-step FFN, LayerNorm) -> Linear 64 -> 198 -> log-softmax.
// fp32 operands and fp32 accumulation throughout (the FFN products on the exact f32-input MFMA, the D = 64 products on plain FMA: both
// are k-ordered fmaf chains).  Every row of the batch is computed as if it were alone: keys and conv taps
// outside [0, 4 n_b) of the row do not exist, nothing behind 4 n_b is read, frames there are written as 0.0 in the output only.
//
// All products share one tile: a workgroup of 256 threads owns 64 frames; the (normalised) activations sit in LDS transposed
// [k][frame] (f32_tile.hpp tile_at), a 64 x 64 block of the weight, transposed to [k][n] at finalize, sits next to them.  The D = 64 products
// (tile_mm): thread (rg, cg) accumulates frames 4 rg .. 4 rg + 3 x columns 4 cg .. 4 cg + 3 from two 16-byte LDS reads per k (the
// activation read is a broadcast).  The FFN products, 93 % of the flops (f32_tile.hpp mfma_k64): wave w owns one 32 x 32 block.
//   asr_ffn      LN, then 16 slices of 64 hidden units: W1 slice, SiLU into LDS, W2 slice into the running output; the hidden
//                activations never leave the CU.  Epilogue: x + 0.5 (. + b2), and for ffn2 the layer's final LayerNorm.
//                138 us against 186 us on the FMA tile at 32 rows x 300 frames, the same bits.
//   asr_qkv      LN + in-projection (q already times 0.5 = 1 / sqrt(4): exact)
//   asr_attn     workgroup = (256 queries, head, row): the head's K and V in LDS (<= 900 x 4 floats each), one query per lane, two passes
//   asr_proj     out-projection + residual
//   asr_conv     56 frames + 4 halo frames either side: LN, pointwise 64 -> 128, GLU, depthwise k = 9, BatchNorm (folded), SiLU,
//                pointwise 64 -> 64, residual.  Reads halo frames other workgroups own: input and output are different buffers.
//   asr_head     projection to 198 classes (4 blocks of 64, zero padded) + log-softmax on the register tile
// No atomics, every sum in a fixed order that does not depend on the batch: results repeat bit for bit, alone or in a batch.
#include "f32_tile.hpp"
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int A_NT = 256, A_TM = 64, A_LD = 64;
constexpr int A_D = 64, A_FF = 1024, A_C = 198, A_HEADS = 16, A_CONV_OUT = 56, A_HALO = 4;
constexpr float A_EPS = 1e-5f;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);   // (a + b == b + a: every lane ends with the same bits)
    return v;
}

__device__ __forceinline__ float ln_lane(float v, float g, float be) {
    const float mean = wave_sum(v) * (1.0f / 64.0f);
    const float d = v - mean;
    const float var = wave_sum(d * d) * (1.0f / 64.0f);
    return d * (1.0f / sqrtf(var + A_EPS)) * g + be;
}

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }

// frames [t0, t0 + 64) of one batch row (rows of 64 floats) -> aT[k][frame]; frames outside [0, tb) become zeros.  LN: LayerNorm first
template <bool LN>
__device__ __forceinline__ void stage_rows(float* aT, const float* xrow, int t0, int tb, const float* g, const float* be) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float gg = LN ? g[lane] : 0.f, bb = LN ? be[lane] : 0.f;
    for (int r = w; r < A_TM; r += A_NT / 64) {
        const int t = t0 + r;
        float v = 0.f;
        if (t >= 0 && t < tb) {   // (uniform per wave)
            v = xrow[(long)t * A_D + lane];
            if (LN) v = ln_lane(v, gg, bb);
        }
        aT[tile_at<A_LD>(lane, r)] = v;
    }
}

__device__ __forceinline__ void load_w(float* wS, const float* __restrict__ src) {
    for (int i = threadIdx.x; i < A_D * A_D / 4; i += A_NT)
        reinterpret_cast<float4*>(wS)[i] = reinterpret_cast<const float4*>(src)[i];
}

__device__ __forceinline__ void tile_mm(const float* aT, const float* wS, int rg, int cg, float (&acc)[4][4]) {
#pragma unroll 8
    for (int k = 0; k < A_D; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(aT + tile_at<A_LD>(k, 4 * rg));
        const float4 w = *reinterpret_cast<const float4*>(wS + k * A_D + 4 * cg);
        const float av[4] = {a.x, a.y, a.z, a.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], wv[j], acc[i][j]);
    }
}

__device__ __forceinline__ void zero_acc(float (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
}

__global__ __launch_bounds__(A_NT) void asr_upsample_kernel(const float* __restrict__ x, const int* __restrict__ n_len, int N,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y) {
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N);
    const int i = blockIdx.x * A_NT + threadIdx.x, t = i >> 6, c = i & 63;
    if (t >= tb) return;
    y[((long)b * T + t) * A_D + c] = x[((long)b * N + (t >> 2)) * A_D + c] * w[c * 4 + (t & 3)] + bias[c];
}

// wave w owns the 32 x 32 block (frames 32 (w >> 1) .., columns 32 (w & 1) ..) of both products
template <bool FINAL_LN>
__global__ __launch_bounds__(A_NT) void asr_ffn_kernel(const float* xin, float* xout /* ffn1: in place */,
                                                       const int* __restrict__ n_len, int N, AsrFfnW w, const float* __restrict__ fg,
                                                       const float* __restrict__ fb) {
    __shared__ __attribute__((aligned(16))) float aT[A_D * A_LD], hT[A_D * A_LD], w1s[A_D * A_D], w2s[A_D * A_D];
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), t0 = blockIdx.x * A_TM;
    if (t0 >= tb) return;   // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f0 = 32 * (wv >> 1), n0 = 32 * (wv & 1), col = n0 + (lane & 31), rbase = f0 + 4 * (lane >> 5);
    const float* const xrow = xin + (long)b * T * A_D;
    stage_rows<true>(aT, xrow, t0, tb, w.ln_w, w.ln_b);
    f32x16 out;
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = 0.f;
    for (int s = 0; s < A_FF / A_D; ++s) {
        load_w(w1s, w.w1t + (long)s * A_D * A_D);
        load_w(w2s, w.w2t + (long)s * A_D * A_D);
        __syncthreads();
        f32x16 h;
#pragma unroll
        for (int i = 0; i < 16; ++i) h[i] = 0.f;
        mfma_k64<A_LD>(aT, f0 + (lane & 31), w1s, 0, n0, lane, h);
        const float b1 = w.b1[s * A_D + col];
#pragma unroll
        for (int g = 0; g < 4; ++g)   // registers 4 g .. 4 g + 3: frames rbase + 8 g .. + 3 of hidden unit col
            *reinterpret_cast<float4*>(hT + tile_at<A_LD>(col, rbase + 8 * g)) =
                make_float4(silu(h[4 * g] + b1), silu(h[4 * g + 1] + b1), silu(h[4 * g + 2] + b1), silu(h[4 * g + 3] + b1));
        __syncthreads();
        mfma_k64<A_LD>(hT, f0 + (lane & 31), w2s, 0, n0, lane, out);
        __syncthreads();   // the next slice overwrites w1s / w2s / hT
    }
    const float b2 = w.b2[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = f0 + tile_row(i, lane), t = t0 + r;
        const float res = t < tb ? xrow[(long)t * A_D + col] : 0.f;
        const float y = fmaf(0.5f, out[i] + b2, res);
        if (FINAL_LN) hT[r * A_LD + col] = y;   // row-major now
        else if (t < tb) xout[((long)b * T + t) * A_D + col] = y;
    }
    if (FINAL_LN) {
        __syncthreads();
        const float gg = fg[lane], bb = fb[lane];
        for (int r = wv; r < A_TM; r += A_NT / 64) {
            const int t = t0 + r;
            if (t >= tb) break;   // (uniform per wave)
            xout[((long)b * T + t) * A_D + lane] = ln_lane(hT[r * A_LD + lane], gg, bb);
        }
    }
}

__global__ __launch_bounds__(A_NT) void asr_qkv_kernel(const float* __restrict__ xin, const int* __restrict__ n_len, int N,
                                                       const float* __restrict__ g, const float* __restrict__ be,
                                                       const float* __restrict__ wt, const float* __restrict__ bias,
                                                       float* __restrict__ qkv) {
    __shared__ __attribute__((aligned(16))) float aT[A_D * A_LD], wS[A_D * A_D];
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), t0 = blockIdx.x * A_TM;
    if (t0 >= tb) return;
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    stage_rows<true>(aT, xin + (long)b * T * A_D, t0, tb, g, be);
    for (int ch = 0; ch < 3; ++ch) {
        load_w(wS, wt + (long)ch * A_D * A_D);
        __syncthreads();
        float acc[4][4];
        zero_acc(acc);
        tile_mm(aT, wS, rg, cg, acc);
        const float4 bv = *reinterpret_cast<const float4*>(bias + ch * A_D + 4 * cg);
        const float sc = ch == 0 ? 0.5f : 1.0f;   // 1 / sqrt(head dim 4)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + 4 * rg + i;
            if (t < tb)
                *reinterpret_cast<float4*>(qkv + ((long)b * T + t) * (3 * A_D) + ch * A_D + 4 * cg) =
                    make_float4((acc[i][0] + bv.x) * sc, (acc[i][1] + bv.y) * sc, (acc[i][2] + bv.z) * sc, (acc[i][3] + bv.w) * sc);
        }
        __syncthreads();
    }
}

constexpr int AT_MAXT = 900;

__global__ __launch_bounds__(A_NT) void asr_attn_kernel(const float* __restrict__ qkv, const int* __restrict__ n_len, int N,
                                                        float* __restrict__ o) {
    __shared__ float4 ks[AT_MAXT], vs[AT_MAXT];
    const int b = blockIdx.z, h = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), q0 = blockIdx.x * A_NT;
    if (q0 >= tb) return;   // (uniform)
    const float* const base = qkv + (long)b * T * (3 * A_D) + 4 * h;
    for (int t = threadIdx.x; t < tb; t += A_NT) {
        ks[t] = *reinterpret_cast<const float4*>(base + (long)t * (3 * A_D) + A_D);
        vs[t] = *reinterpret_cast<const float4*>(base + (long)t * (3 * A_D) + 2 * A_D);
    }
    __syncthreads();
    const int qi = q0 + threadIdx.x;
    if (qi >= tb) return;
    const float4 q = *reinterpret_cast<const float4*>(base + (long)qi * (3 * A_D));
    float m = -INFINITY;
    for (int t = 0; t < tb; ++t) {
        const float4 k = ks[t];
        m = fmaxf(m, fmaf(q.w, k.w, fmaf(q.z, k.z, fmaf(q.y, k.y, q.x * k.x))));
    }
    float l = 0.f, ox = 0.f, oy = 0.f, oz = 0.f, ow = 0.f;
    for (int t = 0; t < tb; ++t) {
        const float4 k = ks[t], v = vs[t];
        const float p = expf(fmaf(q.w, k.w, fmaf(q.z, k.z, fmaf(q.y, k.y, q.x * k.x))) - m);
        l += p;
        ox = fmaf(p, v.x, ox); oy = fmaf(p, v.y, oy); oz = fmaf(p, v.z, oz); ow = fmaf(p, v.w, ow);
    }
    const float inv = 1.0f / l;
    *reinterpret_cast<float4*>(o + ((long)b * T + qi) * A_D + 4 * h) = make_float4(ox * inv, oy * inv, oz * inv, ow * inv);
}

// x (+)= o Wo^T + bo, in place (a workgroup reads only the frames it writes)
__global__ __launch_bounds__(A_NT) void asr_proj_kernel(const float* __restrict__ o, const int* __restrict__ n_len, int N,
                                                        const float* __restrict__ wt, const float* __restrict__ bias,
                                                        float* __restrict__ x) {
    __shared__ __attribute__((aligned(16))) float aT[A_D * A_LD], wS[A_D * A_D];
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), t0 = blockIdx.x * A_TM;
    if (t0 >= tb) return;
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    stage_rows<false>(aT, o + (long)b * T * A_D, t0, tb, nullptr, nullptr);
    load_w(wS, wt);
    __syncthreads();
    float acc[4][4];
    zero_acc(acc);
    tile_mm(aT, wS, rg, cg, acc);
    const float4 bv = *reinterpret_cast<const float4*>(bias + 4 * cg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * rg + i;
        if (t >= tb) continue;
        float4* const p = reinterpret_cast<float4*>(x + ((long)b * T + t) * A_D + 4 * cg);
        const float4 r = *p;
        *p = make_float4((acc[i][0] + bv.x) + r.x, (acc[i][1] + bv.y) + r.y, (acc[i][2] + bv.z) + r.z, (acc[i][3] + bv.w) + r.w);
    }
}

__global__ __launch_bounds__(A_NT) void asr_conv_kernel(const float* __restrict__ xin, float* __restrict__ xout,
                                                        const int* __restrict__ n_len, int N, AsrConvW w) {
    __shared__ __attribute__((aligned(16))) float aT[A_D * A_LD], gb[A_TM * A_LD], wS[A_D * A_D];
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), c0 = blockIdx.x * A_CONV_OUT;
    if (c0 >= tb) return;
    const int t0 = c0 - A_HALO;   // tile row r <-> frame t0 + r; rows [4, 60) are this workgroup's outputs
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4, lane = tid & 63, wv = tid >> 6;
    const float* const xrow = xin + (long)b * T * A_D;
    stage_rows<true>(aT, xrow, t0, tb, w.ln_w, w.ln_b);
    load_w(wS, w.pw1t);
    __syncthreads();
    float a[4][4], gt[4][4];
    zero_acc(a);
    tile_mm(aT, wS, rg, cg, a);
    __syncthreads();
    load_w(wS, w.pw1t + A_D * A_D);
    __syncthreads();
    zero_acc(gt);
    tile_mm(aT, wS, rg, cg, gt);
    {
        const float4 ba = *reinterpret_cast<const float4*>(w.pw1b + 4 * cg), bg = *reinterpret_cast<const float4*>(w.pw1b + A_D + 4 * cg);
        const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + 4 * rg + i;
            const bool live = t >= 0 && t < tb;   // the depthwise conv sees zeros outside the row
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = live ? (a[i][j] + bav[j]) * (1.0f / (1.0f + expf(-(gt[i][j] + bgv[j])))) : 0.f;
            *reinterpret_cast<float4*>(gb + (4 * rg + i) * A_LD + 4 * cg) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
    __syncthreads();   // gb complete; everyone is done with aT and wS
    load_w(wS, w.pw2t);
    {
        float dw[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) dw[j] = w.dw_w[lane * 9 + j];
        const float db = w.dw_b[lane], sc = w.bn_scale[lane], sh = w.bn_shift[lane];
        for (int r = wv; r < A_TM; r += A_NT / 64) {
            float y = 0.f;
            if (r >= A_HALO && r < A_HALO + A_CONV_OUT) {
                float d = db;
#pragma unroll
                for (int j = 0; j < 9; ++j) d = fmaf(gb[(r - A_HALO + j) * A_LD + lane], dw[j], d);
                y = silu(fmaf(d, sc, sh));
            }
            aT[tile_at<A_LD>(lane, r)] = y;
        }
    }
    __syncthreads();
    float acc[4][4];
    zero_acc(acc);
    tile_mm(aT, wS, rg, cg, acc);
    const float4 bv = *reinterpret_cast<const float4*>(w.pw2b + 4 * cg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 4 * rg + i, t = t0 + r;
        if (r < A_HALO || r >= A_HALO + A_CONV_OUT || t >= tb) continue;
        const float4 x4 = *reinterpret_cast<const float4*>(xrow + (long)t * A_D + 4 * cg);
        *reinterpret_cast<float4*>(xout + ((long)b * T + t) * A_D + 4 * cg) =
            make_float4((acc[i][0] + bv.x) + x4.x, (acc[i][1] + bv.y) + x4.y, (acc[i][2] + bv.z) + x4.z, (acc[i][3] + bv.w) + x4.w);
    }
}

// logits in registers: thread (rg, cg) holds frames 4 rg .. + 3 x classes 64 ch + 4 cg .. + 3 of all four blocks; the 16 threads of a frame
// group are 16 consecutive lanes, so a frame's maximum and sum are xor butterflies over 8, 4, 2, 1 (every lane ends with the same bits)
__global__ __launch_bounds__(A_NT) void asr_head_kernel(const float* __restrict__ x, const int* __restrict__ n_len, int N,
                                                        const float* __restrict__ wt, const float* __restrict__ bias,
                                                        float* __restrict__ logp) {
    __shared__ __attribute__((aligned(16))) float aT[A_D * A_LD], wS[A_D * A_D];
    const int b = blockIdx.y, T = 4 * N, tb = 4 * row_len(n_len, b, N), t0 = blockIdx.x * A_TM;
    const int tid = threadIdx.x, cg = tid & 15, rg = tid >> 4;
    float acc[4][4][4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) zero_acc(acc[ch]);
    if (t0 < tb) {   // (uniform)
        stage_rows<false>(aT, x + (long)b * T * A_D, t0, tb, nullptr, nullptr);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            load_w(wS, wt + (long)ch * A_D * A_D);
            __syncthreads();
            tile_mm(aT, wS, rg, cg, acc[ch]);
            const float4 bv = *reinterpret_cast<const float4*>(bias + ch * A_D + 4 * cg);
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc[ch][i][0] += bv.x; acc[ch][i][1] += bv.y; acc[ch][i][2] += bv.z; acc[ch][i][3] += bv.w; }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * rg + i;
        float m = -INFINITY;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ch * A_D + 4 * cg + j < A_C) m = fmaxf(m, acc[ch][i][j]);
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float s = 0.f;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ch * A_D + 4 * cg + j < A_C) s += expf(acc[ch][i][j] - m);
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        const float ls = logf(s);
        if (t >= T) continue;
        float* const orow = logp + ((long)b * T + t) * A_C;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = ch * A_D + 4 * cg + j;
                if (c < A_C) orow[c] = t < tb ? (acc[ch][i][j] - m) - ls : 0.f;   // behind the row's end: zeros
            }
    }
}

}  // namespace

size_t asr_ws_bytes(int B, int N) {
    const size_t rows = (size_t)B * 4 * N;
    return 3 * up256(rows * A_D * 4) + up256(rows * 3 * A_D * 4);
}

// launch order: upsample; per layer ffn1, qkv, attn, proj, conv, ffn2; head
size_t asr_tap_bytes(int B, int N, int slot) {
    if (slot < 0 || slot >= ASR_TAPS) return 0;
    const size_t rows = (size_t)B * 4 * N;
    if (slot == ASR_TAPS - 1) return rows * A_C * 4;
    return (slot - 1) % 6 == 1 && slot > 0 ? rows * 3 * A_D * 4 : rows * A_D * 4;
}

hipError_t launch_asr_logprobs(const AsrW& w, const float* x, const int* n_len, int B, int N, void* ws, float* logp, hipStream_t st,
                               const ScorerTaps* taps) {
    if (B < 1 || N < 1 || 4 * N > AT_MAXT) return hipErrorInvalidValue;
    const int T = 4 * N;
    const size_t rows = (size_t)B * T;
    char* p = static_cast<char*>(ws);
    float* xa = reinterpret_cast<float*>(p); p += up256(rows * A_D * 4);
    float* xb = reinterpret_cast<float*>(p); p += up256(rows * A_D * 4);
    float* ob = reinterpret_cast<float*>(p); p += up256(rows * A_D * 4);
    float* qkv = reinterpret_cast<float*>(p);
    const dim3 wg(A_NT), tiles((T + A_TM - 1) / A_TM, B);
    const double fr = (double)rows;
    int slot = 0;
    hipError_t te = hipSuccess;
    auto tap = [&](const float* buf) {   // (tests only) what the launch just enqueued wrote, into its slot
        if (!taps) return;
        const hipError_t e = hipMemcpyAsync(taps->base + taps->off[slot], buf, asr_tap_bytes(B, N, slot), hipMemcpyDeviceToDevice, st);
        if (te == hipSuccess) te = e;
        ++slot;
    };
    {
        ProfScope ps(st, "asr_upsample", 2.0 * fr * A_D, 5.0 * fr * A_D);
        hipLaunchKernelGGL(asr_upsample_kernel, dim3((T * A_D + A_NT - 1) / A_NT, B), wg, 0, st, x, n_len, N, w.up_w, w.up_b, xa);
    }
    tap(xa);
    for (int l = 0; l < 7; ++l) {
        const AsrLayerW& L = w.layer[l];
        {
            ProfScope ps(st, "asr_ffn", 4.0 * fr * A_D * A_FF, 8.0 * fr * A_D);
            hipLaunchKernelGGL((asr_ffn_kernel<false>), tiles, wg, 0, st, xa, xa, n_len, N, L.ffn1, nullptr, nullptr);
        }
        tap(xa);
        {
            ProfScope ps(st, "asr_qkv", 6.0 * fr * A_D * A_D, 16.0 * fr * A_D);
            hipLaunchKernelGGL(asr_qkv_kernel, tiles, wg, 0, st, xa, n_len, N, L.aln_w, L.aln_b, L.wqkv_t, L.bqkv, qkv);
        }
        tap(qkv);
        {
            ProfScope ps(st, "asr_attn", 4.0 * fr * T * A_D, 16.0 * fr * A_D);
            hipLaunchKernelGGL(asr_attn_kernel, dim3((T + A_NT - 1) / A_NT, A_HEADS, B), wg, 0, st, qkv, n_len, N, ob);
        }
        tap(ob);
        {
            ProfScope ps(st, "asr_proj", 2.0 * fr * A_D * A_D, 12.0 * fr * A_D);
            hipLaunchKernelGGL(asr_proj_kernel, tiles, wg, 0, st, ob, n_len, N, L.wo_t, L.bo, xa);
        }
        tap(xa);
        {
            ProfScope ps(st, "asr_conv", 6.0 * fr * A_D * A_D, 8.0 * fr * A_D);
            hipLaunchKernelGGL(asr_conv_kernel, dim3((T + A_CONV_OUT - 1) / A_CONV_OUT, B), wg, 0, st, xa, xb, n_len, N, L.conv);
        }
        tap(xb);
        {
            ProfScope ps(st, "asr_ffn", 4.0 * fr * A_D * A_FF, 8.0 * fr * A_D);
            hipLaunchKernelGGL((asr_ffn_kernel<true>), tiles, wg, 0, st, xb, xa, n_len, N, L.ffn2, L.fln_w, L.fln_b);
        }
        tap(xa);
    }
    {
        ProfScope ps(st, "asr_head", 2.0 * fr * A_D * 256, 4.0 * fr * (A_D + A_C));
        hipLaunchKernelGGL(asr_head_kernel, tiles, wg, 0, st, xa, n_len, N, w.proj_t, w.proj_b, logp);
    }
    tap(logp);
    const hipError_t le = hipGetLastError();
    return le != hipSuccess ? le : te;
}
