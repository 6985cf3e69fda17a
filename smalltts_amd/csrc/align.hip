// Word timings from the DiT's text attention (DESIGN 'Word timings'), gfx950.
//
// attn_text_mass: launched right behind launch_attention_img for a selected (step, layer).  It reads what that kernel just read — the
// Q / self-K operand images, the layer's cross-K image and the three key masks (AttnImg, kernels.hpp; layout in the header of
// attention_img.hip) — recomputes the softmax of every valid frame over ALL valid keys in fp32 (the logits are already scaled in the
// Q image) and adds the probabilities of the TEXT keys of the selected heads into the caller's fp32 buffer mass (B, N, P):
//     mass[b][n][p] (+)= scale * sum_{h selected} softmax_k(q_n . k)[text key p]
// The first tap of a sampler call stores, later taps add; scale = 1 / (number of selected (step, layer, head) triples), so the buffer ends
// as their mean and a frame's row sums to at most 1.  Exactly 0 for frames the row mask excludes, for masked text columns and for rows
// whose keys are all masked.
//   workgroup = (4-frame tile, batch row), 256 threads, heads walked in ascending order;
//   logits: thread = key position (stride 256), its whole key row in flight as independent 16-byte loads, the 4 queries as fp32 in LDS
//   (broadcast reads), dot products in dimension order;
//   softmax statistics: wave w owns query w (lane-strided partials, xor butterfly: every lane ends with the same bits);
//   accumulation: thread tid owns elements tid, tid + 256, ... of the tile's [4][P] block in LDS and alone writes them to mass.
// No atomics, no order that depends on scheduling: two runs return the same bits whatever else the chip is doing.  Plain VALU + LDS:
// one tap is 0.14 GFLOP at the bench shape (8 rows x 75 frames x 120 keys x 8 heads x 120 dims) and runs only when the caller asks for timings.
//
// align_path: monotone alignment of one batch row per workgroup by an anti-diagonal wavefront DP, back-pointers in LDS (225 x 198
// bytes), thread = token.  cost c[n][p] = 1 - mass[b][n][p] (one fp32 subtraction), D[n][p] = c[n][p] + min(D[n-1][p-1], D[n-1][p],
// D[n][p-1]) (one fp32 addition), ties prefer the diagonal, then (n-1, p), then (n, p-1); the path runs from (0, p0) to (n_b - 1, p1 - 1).
// Single fp32 operations in a fixed order: a numpy float32 restatement reproduces spans and score bit for bit.
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int TM_QT = 4, TM_NT = 256;

// eight consecutive operand values from their raw 16-byte pieces (hi, and lo for the split format)
template <int PREC>
__device__ __forceinline__ void decode_img8(const uint4& hi, const uint4& lo, float (&v)[8]) {
    const unsigned h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (PREC == PREC_F16) {
            const half2_t p = __builtin_bit_cast(half2_t, h[j]);
            v[2 * j] = (float)p[0]; v[2 * j + 1] = (float)p[1];
        } else {
            v[2 * j] = __uint_as_float(h[j] << 16); v[2 * j + 1] = __uint_as_float(h[j] & 0xffff0000u);
            if constexpr (PREC == PREC_BF16X3) {   // hi + lo carries 16 mantissa bits: exact in fp32
                v[2 * j] += __uint_as_float(l[j] << 16); v[2 * j + 1] += __uint_as_float(l[j] & 0xffff0000u);
            }
        }
    }
}

template <int PREC, int DHP>
__global__ __launch_bounds__(TM_NT) void attn_text_mass_kernel(AttnImg a, float* __restrict__ mass, unsigned heads, float scale, int first) {
    extern __shared__ __attribute__((aligned(16))) float tm_smem[];
    constexpr int NPC = DHP / 8;                     // 16-byte pieces per image row
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, q0 = blockIdx.x * TM_QT;
    const int N = a.N, Np = a.Np, Rp = a.Rp, Cp = a.Cp, P = a.P, R = a.R;
    const int Kpos = Np + Cp, T0 = Np + Rp;          // key positions: [0, Np) self | [Np, T0) reference | [T0, Kpos) text
    float* const qs = tm_smem;                       // [QT][DHP]   the tile's queries, fp32
    float* const sl = qs + TM_QT * DHP;              // [QT][Kpos]  logits (-inf: key masked or padding)
    float* const acc = sl + TM_QT * Kpos;            // [QT][P]     sum over the selected heads of the text probabilities
    float* const stat = acc + TM_QT * P;             // [2][QT]     row maximum, 1 / row sum

    for (int i = tid; i < TM_QT * P; i += TM_NT) acc[i] = 0.f;
    // key validity does not depend on the head: one bit per key this thread owns (keys tid, tid + 256, ...; the launcher bounds Kpos)
    unsigned okbits = 0;
    for (int kp = tid, i = 0; kp < Kpos; kp += TM_NT, ++i) {
        bool ok;
        if (kp < Np) {
            ok = kp < N && (!a.mask_self || a.mask_self[(long)b * N + kp]);
        } else {
            const int j = kp - Np;
            if (j < Rp) ok = j < R && (!a.mask_ref || a.mask_ref[(long)b * R + j]);
            else ok = j - Rp < P && (!a.mask_text || a.mask_text[(long)b * P + (j - Rp)]);
        }
        okbits |= (ok ? 1u : 0u) << i;
    }
    for (int h = 0; h < a.H; ++h) {
        if (!((heads >> h) & 1u)) continue;          // (uniform)
        const long bh = (long)b * a.H + h;
        __syncthreads();                             // the previous head is done with qs / sl / stat
        for (int i = tid; i < TM_QT * NPC; i += TM_NT) {
            const int q = i / NPC, c = i % NPC;
            int n = q0 + q;
            n = n < N ? n : N - 1;
            const long off = (bh * N + n) * DHP + c * 8;
            const uint4 hi = *reinterpret_cast<const uint4*>(a.q + off);
            uint4 lo = make_uint4(0u, 0u, 0u, 0u);
            if constexpr (PREC == PREC_BF16X3) lo = *reinterpret_cast<const uint4*>(a.q_lo + off);
            float v[8];
            decode_img8<PREC>(hi, lo, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) qs[q * DHP + c * 8 + j] = v[j];
        }
        __syncthreads();
        for (int kp = tid, i = 0; kp < Kpos; kp += TM_NT, ++i) {
            const bf16_t *kh, *kl;
            long ro;
            if (kp < Np) {
                kh = a.k; kl = a.k_lo; ro = (bh * N + (kp < N ? kp : N - 1)) * DHP;   // (pad rows: any readable row, masked out)
            } else {
                kh = a.kc; kl = a.kc_lo; ro = (bh * Cp + (kp - Np)) * DHP;
            }
            // the whole key row goes out as independent 16-byte loads before the first product waits for one
            uint4 rh[NPC], rl[NPC];
#pragma unroll
            for (int c = 0; c < NPC; ++c) {
                rh[c] = *reinterpret_cast<const uint4*>(kh + ro + c * 8);
                if constexpr (PREC == PREC_BF16X3) rl[c] = *reinterpret_cast<const uint4*>(kl + ro + c * 8);
                else rl[c] = make_uint4(0u, 0u, 0u, 0u);
            }
            float dot[TM_QT];
#pragma unroll
            for (int q = 0; q < TM_QT; ++q) dot[q] = 0.f;
#pragma unroll
            for (int c = 0; c < NPC; ++c) {
                float kv[8];
                decode_img8<PREC>(rh[c], rl[c], kv);
#pragma unroll
                for (int q = 0; q < TM_QT; ++q) {
                    const float4 qa = *reinterpret_cast<const float4*>(qs + q * DHP + c * 8);
                    const float4 qb = *reinterpret_cast<const float4*>(qs + q * DHP + c * 8 + 4);
                    float d = dot[q];
                    d = fmaf(kv[0], qa.x, d); d = fmaf(kv[1], qa.y, d); d = fmaf(kv[2], qa.z, d); d = fmaf(kv[3], qa.w, d);
                    d = fmaf(kv[4], qb.x, d); d = fmaf(kv[5], qb.y, d); d = fmaf(kv[6], qb.z, d); d = fmaf(kv[7], qb.w, d);
                    dot[q] = d;
                }
            }
            const bool ok = (okbits >> i) & 1u;
#pragma unroll
            for (int q = 0; q < TM_QT; ++q) sl[q * Kpos + kp] = ok ? dot[q] : -INFINITY;
        }
        __syncthreads();
        for (int q = w; q < TM_QT; q += TM_NT / 64) {
            const float* const row = sl + q * Kpos;
            float m = -INFINITY;
            for (int kp = lane; kp < Kpos; kp += 64) m = fmaxf(m, row[kp]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            float l = 0.f;
            if (m != -INFINITY)
                for (int kp = lane; kp < Kpos; kp += 64) {
                    const float s = row[kp];
                    l += s != -INFINITY ? expf(s - m) : 0.f;
                }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) l += __shfl_xor(l, o, 64);   // (a + b == b + a: every lane holds the same bits)
            if (lane == 0) {
                stat[q] = m;
                stat[TM_QT + q] = l > 0.f ? 1.0f / l : 0.f;
            }
        }
        __syncthreads();
        for (int i = tid; i < TM_QT * P; i += TM_NT) {
            const int q = i / P, p = i % P;
            const float s = sl[q * Kpos + T0 + p];
            acc[i] += s != -INFINITY ? expf(s - stat[q]) * stat[TM_QT + q] : 0.f;
        }
    }
    // (each element of acc was only ever touched by the thread that stores it)
    for (int i = tid; i < TM_QT * P; i += TM_NT) {
        const int q = i / P, p = i % P, n = q0 + q;
        if (n >= N) continue;
        const bool live = !a.mask_self || a.mask_self[(long)b * N + n];
        const long o = ((long)b * N + n) * P + p;
        const float v = live ? acc[i] * scale : 0.f;
        mass[o] = (first || !live) ? v : mass[o] + v;
    }
}

constexpr int AP_MAXN = 225, AP_MAXP = 198;   // the API's range: 30 s of frames, the phoneme window

__global__ __launch_bounds__(256) void align_path_kernel(const float* __restrict__ mass, int N, int P, const int* __restrict__ n_len,
                                                         const int* __restrict__ p0a, const int* __restrict__ p1a, int* __restrict__ spans,
                                                         float* __restrict__ score) {
    __shared__ unsigned char bp[AP_MAXN * AP_MAXP];   // back-pointer of cell (n, t): 0 diagonal, 1 (n-1, p), 2 (n, p-1)
    __shared__ float dg[3][256];                      // D on the anti-diagonals d, d-1, d-2 (indexed by token)
    __shared__ int sfirst[AP_MAXP], slast[AP_MAXP];
    const int b = blockIdx.x, t = threadIdx.x;
    int nb = n_len[b], p0 = p0a[b], p1 = p1a[b];
    nb = nb < 0 ? 0 : nb > N ? N : nb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int Pw = p1 - p0;
    if (t < P) { sfirst[t] = -1; slast[t] = -1; }
    if (nb > 0 && Pw > 0) {   // (uniform)
        const float* const mrow = mass + (long)b * N * P + p0;
        const int nd = nb + Pw - 1;
        for (int d = 0; d < nd; ++d) {
            float* const cur = dg[d % 3];
            const float* const d1 = dg[(d + 2) % 3];
            const float* const d2 = dg[(d + 1) % 3];
            const int n = d - t;
            if (t < Pw && n >= 0 && n < nb) {
                const float c = 1.0f - mrow[(long)n * P + t];
                const float diag = (t > 0 && n > 0) ? d2[t - 1] : INFINITY;
                const float up = n > 0 ? d1[t] : INFINITY;
                const float left = t > 0 ? d1[t - 1] : INFINITY;
                float best = diag;
                int k = 0;
                if (up < best) { best = up; k = 1; }
                if (left < best) { best = left; k = 2; }
                cur[t] = (n == 0 && t == 0) ? c : c + best;
                bp[n * AP_MAXP + t] = (unsigned char)k;
            }
            __syncthreads();
        }
        if (t == 0) {
            score[b] = dg[(nd - 1) % 3][Pw - 1];
            int n = nb - 1, p = Pw - 1;
            slast[p0 + p] = n;
            while (n > 0 || p > 0) {
                int k = bp[n * AP_MAXP + p];
                k = n == 0 ? 2 : p == 0 ? 1 : k;   // the only move a border cell has (also what the forward pass stored for finite costs): n + p falls every turn
                if (k == 1) { --n; continue; }
                sfirst[p0 + p] = n;
                --p;
                if (k == 0) --n;
                slast[p0 + p] = n;
            }
            sfirst[p0] = 0;
        }
    } else if (t == 0) {
        score[b] = 0.f;
    }
    __syncthreads();
    if (t < P) {
        spans[((long)b * P + t) * 2] = sfirst[t];
        spans[((long)b * P + t) * 2 + 1] = slast[t];
    }
}

}  // namespace

static size_t attn_text_mass_lds(const AttnImg& a) {
    const int dhp = a.dh <= 64 ? 64 : 128;
    return sizeof(float) * ((size_t)TM_QT * (dhp + a.Np + a.Cp + a.P) + 2 * TM_QT);
}

hipError_t launch_attn_text_mass(const AttnImg& a, float* mass, int rows, unsigned heads, float scale, int first, hipStream_t st) {
    if (!mass || !a.kc || a.P <= 0 || a.N <= 0 || rows <= 0 || rows > a.B || a.H > 32 || !(heads & (a.H >= 32 ? ~0u : (1u << a.H) - 1u)))
        return hipErrorInvalidValue;
    if (a.dh > 128 || (a.Np % 8) || (a.Cp % 8) || (a.Rp % 8) || a.Np < a.N || a.Cp < a.Rp + a.P) return hipErrorInvalidValue;
    const size_t lds = attn_text_mass_lds(a);
    if (lds > 64 * 1024 || a.Np + a.Cp > 32 * TM_NT) return hipErrorInvalidValue;   // (Ktot + P beyond ~4000 keys: outside every shape the API produces)
    const int dhp = a.dh <= 64 ? 64 : 128;
    int nh = 0;
    for (int h = 0; h < a.H; ++h) nh += (heads >> h) & 1u;
    const double kt = a.N + a.R + a.P;
    ProfScope ps(st, "attn_text_mass", 2.0 * rows * nh * a.N * kt * a.dh, (a.prec == PREC_BF16X3 ? 4.0 : 2.0) * rows * nh * (a.N + kt) * dhp);
    const dim3 grid((a.N + TM_QT - 1) / TM_QT, rows);
#define TM_GO(PREC, DHP) hipLaunchKernelGGL((attn_text_mass_kernel<PREC, DHP>), grid, dim3(TM_NT), lds, st, a, mass, heads, scale, first)
    switch (a.prec) {
        case PREC_BF16X3: if (dhp == 64) TM_GO(PREC_BF16X3, 64); else TM_GO(PREC_BF16X3, 128); break;
        case PREC_F16: if (dhp == 64) TM_GO(PREC_F16, 64); else TM_GO(PREC_F16, 128); break;
        case PREC_BF16: if (dhp == 64) TM_GO(PREC_BF16, 64); else TM_GO(PREC_BF16, 128); break;
        default: return hipErrorInvalidValue;
    }
#undef TM_GO
    return hipGetLastError();
}

hipError_t launch_align_path(const float* mass, int B, int N, int P, const int* n_len, const int* p0, const int* p1, int* spans, float* score,
                             hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (N < 1 || P < 1 || N > AP_MAXN || P > AP_MAXP) return hipErrorInvalidValue;
    ProfScope ps(st, "align_path", 4.0 * B * N * P, 4.0 * B * N * P);
    hipLaunchKernelGGL(align_path_kernel, dim3(B), dim3(256), 0, st, mass, N, P, n_len, p0, p1, spans, score);
    return hipGetLastError();
}
