// The best CTC path of a long recording (DESIGN '8m. Long alignment'), gfx950.  No weights.
//
// ctc_align_long: smtts_ctc_align's definition (include/smalltts_hip.h, that entry's block) for rows whose lattice fits neither one
// thread per state nor LDS: up to 65536 frames and 16383 tokens (S = 2 L + 1 <= 32767 extended states).  One workgroup per row.
//   forward  Thread i owns the CL_K = 32 states [32 i, 32 i + 32): their delta, their 16 labels and their skip bits stay in registers
//            for the whole row, delta never goes to memory.  State s reads delta_{t-1} of s, s - 1 and, where it may skip, s - 2.  A
//            thread's first state is even (a blank: no skip), so from outside it needs only the top value of its left neighbour (state
//            32 i - 1: one step below its state 0, two below its state 1); it travels through xch[2][thread] in LDS, double-buffered,
//            one barrier per step, the trip count the row's frame count.  The states are updated in place from the top one down
//            (state k reads k - 1 and k - 2, not yet overwritten).  The emission rows come through ctc_score's ring: lp_t[0 .. C) in
//            LDS, the next CL_CH rows in flight as independent loads across the current CL_CH steps.  No exp, no log.
//   moves    2 bits per state and step; a thread packs those of its 32 states into two words and stores them as one 8-byte vector store
//            into the workspace table [t][thread] (coalesced, no atomics, no cross-lane packing).  512 MiB per row at the limits.
//   trace    T dependent loads from HBM would cost a memory latency each.  The state falls by at most 2 per step, so over CL_G = 256
//            steps the trace stays inside the words of ceil(2 G / K) + 1 = 17 neighbouring threads: the workgroup copies that slab
//            (256 x 17 x 8 = 34 816 bytes, independent loads) into LDS, thread 0 walks its 256 steps in LDS, the workgroup stores the
//            256 states to the workspace (u16 state[T]), and so on down to frame 1.
//   outputs  parallel again, as in ctc_align_kernel: thread = frame marks the two ends of every label run straight in spans (one
//            writer each), thread = token sums its tok_logp over its span with t ascending, thread = frame writes frame_tok.
// LDS (static, 35 340 bytes): the slab shares its bytes with the ring (2 x 8 x 256 floats = 16 384) and xch (2 x 1024 floats = 8 192),
// which are dead once the forward pass has ended; + 512 bytes of chunk states + the two end values and the chunk's entry state (12).
#include "kernels.hpp"
#include "prof.hpp"

namespace {

constexpr int CL_K = 32;            // extended states per thread (two 32-bit move words per step)
constexpr int CL_G = 256;           // steps per trace chunk
constexpr int CL_CH = 8;            // steps per ring half = loads in flight per loader thread
constexpr int CL_MAXNT = 1024, CL_MINNT = 256, CL_MAXC = 256;
constexpr int CL_MAXT = 65536, CL_MAXP = 16383;
constexpr int CL_NSL = 2 * CL_G / CL_K + 1;                                   // threads whose words one chunk of the trace can touch
constexpr size_t CL_RING_BYTES = sizeof(float) * 2 * CL_CH * CL_MAXC;         // 16384
constexpr size_t CL_FWD_BYTES = CL_RING_BYTES + sizeof(float) * 2 * CL_MAXNT;    // 24576
constexpr size_t CL_SLAB_BYTES = sizeof(uint2) * CL_G * CL_NSL;               // 34816
constexpr size_t CL_LDS_BYTES = CL_SLAB_BYTES > CL_FWD_BYTES ? CL_SLAB_BYTES : CL_FWD_BYTES;
static_assert(CL_K == 32 && CL_K * CL_MAXNT >= 2 * CL_MAXP + 1, "a thread packs 32 moves into two words; 1024 threads hold every state");

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int cl_words(int P) { return (2 * P + 1 + CL_K - 1) / CL_K; }                      // threads that own a state of a full window
inline size_t cl_off_state(int T, int P) { return al256((size_t)T * cl_words(P) * sizeof(uint2)); }
inline size_t cl_row_bytes(int T, int P) { return cl_off_state(T, P) + al256((size_t)T * sizeof(unsigned short)); }

__device__ __forceinline__ int cl_clamp_tok(int v, int C) { return v < 1 ? 1 : v > C - 1 ? C - 1 : v; }

__global__ __launch_bounds__(CL_MAXNT) void ctc_align_long_kernel(const float* __restrict__ logp, const int* __restrict__ t_len,
                                                                  const int* __restrict__ tokens, const int* __restrict__ p0a,
                                                                  const int* __restrict__ p1a, int T, int P, int C, int W,
                                                                  size_t row_bytes, size_t off_state, int* spans, float* tok_logp,
                                                                  int* frame_tok, float* score, char* ws) {
    __shared__ __attribute__((aligned(16))) char lds[CL_LDS_BYTES];
    __shared__ unsigned short sst[CL_G];
    __shared__ float fin[2];
    __shared__ int sh_q;
    float (*const ring)[CL_CH][CL_MAXC] = reinterpret_cast<float (*)[CL_CH][CL_MAXC]>(lds);
    float (*const xch)[CL_MAXNT] = reinterpret_cast<float (*)[CL_MAXNT]>(lds + CL_RING_BYTES);
    uint2* const slab = reinterpret_cast<uint2*>(lds);   // (after the forward pass)
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    int tb = t_len[b], p0 = p0a[b], p1 = p1a[b];
    tb = tb < 0 ? 0 : tb > T ? T : tb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int L = p1 - p0, S = 2 * L + 1;
    int* const sp = spans + (long)b * P * 2;
    float* const tl = tok_logp + (long)b * P;
    int* const ft = frame_tok ? frame_tok + (long)b * T : nullptr;
    const float* const lrow = logp + (long)b * T * C;
    uint2* const mtab = reinterpret_cast<uint2*>(ws + (size_t)b * row_bytes);                           // [t][thread], t >= 1
    unsigned short* const stt = reinterpret_cast<unsigned short*>(ws + (size_t)b * row_bytes + off_state);   // state[t]
    bool aligned = false;
    if (tb == 0 || L <= 0) {   // (uniform)
        if (tid == 0) score[b] = -INFINITY;
    } else {
        const int base = tid * CL_K;
        const bool active = base < S;   // this thread owns a state of the row; its left neighbour then does too
        unsigned lab4[CL_K / 8] = {};   // label of state base + 2 j + 1 (< 256) at byte j & 3 of word j >> 2; 0 (the blank's column)
                                        // behind the row's last state
        unsigned skipm = 0;             // bit j: skip(base + 2 j + 1)
        {
            const int* const tk = tokens + (long)b * P + p0;
            int prev = active && tid > 0 ? cl_clamp_tok(tk[base / 2 - 1], C) : 0;
#pragma unroll
            for (int j = 0; j < CL_K / 2; ++j) {
                const int s = base + 2 * j + 1;
                int l = 0;
                if (s < S) {
                    l = cl_clamp_tok(tk[s >> 1], C);
                    if (s >= 3 && l != prev) skipm |= 1u << j;
                }
                lab4[j >> 2] |= (unsigned)l << (8 * (j & 3));
                prev = l;
            }
        }
        float d[CL_K];
        const bool loader = tid < C;
        if (loader)
            for (int i = 0; i < CL_CH; ++i) ring[0][i][tid] = i < tb ? lrow[(long)i * C + tid] : 0.f;
        __syncthreads();
        const int nch = (tb + CL_CH - 1) / CL_CH;
        for (int ch = 0; ch < nch; ++ch) {
            const int half = ch & 1, t0 = ch * CL_CH;
            float nxt[CL_CH];
            if (loader) {   // the next chunk's rows: CL_CH loads in flight across this chunk's steps
#pragma unroll
                for (int i = 0; i < CL_CH; ++i) {
                    const int t = t0 + CL_CH + i;
                    nxt[i] = t < tb ? lrow[(long)t * C + tid] : 0.f;
                }
            }
            const int nst = tb - t0 < CL_CH ? tb - t0 : CL_CH;
            for (int i = 0; i < nst; ++i) {
                const int t = t0 + i;
                if (active) {
                    const float* const rr = ring[half][i];
                    const float lpb = rr[0];
                    if (t == 0) {   // (uniform)
#pragma unroll
                        for (int k = 0; k < CL_K; ++k) d[k] = -INFINITY;
                        if (tid == 0) { d[0] = lpb; d[1] = rr[lab4[0] & 255u]; }
                    } else {
                        const float l1 = tid > 0 ? xch[(t + 1) & 1][tid - 1] : -INFINITY;   // delta_{t-1} of state base - 1
                        unsigned m0 = 0, m1 = 0;   // the move of state base + k at bits 2 (k & 15) of word k >> 4
#pragma unroll
                        for (int k = CL_K - 1; k >= 0; --k) {   // top down: d[k - 1] and d[k - 2] still hold step t - 1
                            float v = d[k];
                            unsigned m = 0;
                            const float a = k >= 1 ? d[k >= 1 ? k - 1 : 0] : l1;
                            if (a > v) { v = a; m = 1; }
                            if (k & 1) {
                                if ((skipm >> (k >> 1)) & 1u) {
                                    const float a2 = k >= 2 ? d[k >= 2 ? k - 2 : 0] : l1;   // (k == 1: state base - 1)
                                    if (a2 > v) { v = a2; m = 2; }
                                }
                                v = v + rr[(lab4[k >> 3] >> (8 * ((k >> 1) & 3))) & 255u];
                            } else {
                                v = v + lpb;
                            }
                            d[k] = v;
                            if (k < 16) m0 = (m0 << 2) | m;   // (k descends: k & 15 == 15 ends at the top two bits)
                            else m1 = (m1 << 2) | m;
                        }
                        mtab[(size_t)t * W + tid] = make_uint2(m0, m1);
                    }
                    xch[t & 1][tid] = d[CL_K - 1];
                }
                if (i == nst - 1 && loader) {   // (uniform in i) the other half was last read in the previous chunk, behind a barrier
#pragma unroll
                    for (int j = 0; j < CL_CH; ++j) ring[half ^ 1][j][tid] = nxt[j];
                }
                __syncthreads();
            }
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < CL_K; ++k) {
                if (base + k == S - 2) fin[0] = d[k];
                if (base + k == S - 1) fin[1] = d[k];
            }
        }
        __syncthreads();
        const int e = fin[0] > fin[1] ? S - 2 : S - 1;
        const float sc = e == S - 2 ? fin[0] : fin[1];
        aligned = sc > -INFINITY;   // (uniform; false for NaN)
        if (tid == 0) {
            score[b] = sc;
            sh_q = e;
        }
        if (aligned) {
            __syncthreads();
            for (int thi = tb - 1; thi >= 1; thi -= CL_G) {   // the steps thi ... thi - n + 1 (>= 1), entered in state sh_q
                const int q0 = sh_q;
                const int hi = q0 / CL_K, lo = hi - (CL_NSL - 1) > 0 ? hi - (CL_NSL - 1) : 0;
                const int n = thi < CL_G ? thi : CL_G;
                for (int idx = tid; idx < n * CL_NSL; idx += NT) {   // threads lo ... hi all own states below S: they wrote every step
                    const int g = idx / CL_NSL, j = idx - g * CL_NSL;
                    if (lo + j <= hi) slab[idx] = mtab[(size_t)(thi - g) * W + lo + j];
                }
                __syncthreads();
                if (tid == 0) {   // n dependent LDS reads; the index stays inside [0, q0] and inside the slab whatever the table holds
                    int q = q0;
                    for (int g = 0; g < n; ++g) {
                        sst[g] = (unsigned short)q;
                        const uint2 w = slab[g * CL_NSL + (q / CL_K - lo)];
                        const int k = q & (CL_K - 1);
                        unsigned m = ((k < 16 ? w.x : w.y) >> (2 * (k & 15))) & 3u;
                        m = m > 2u ? 2u : m;
                        q -= (int)m;
                        q = q < 0 ? 0 : q;
                    }
                    sh_q = q;
                }
                __syncthreads();
                for (int g = tid; g < n; g += NT) stt[thi - g] = sst[g];
            }
            if (tid == 0) stt[0] = (unsigned short)sh_q;
        }
    }
    for (int p = tid; p < P; p += NT) {
        sp[2 * p] = -1;
        sp[2 * p + 1] = -1;
    }
    __syncthreads();
    if (aligned) {   // thread = frame: the ends of every label state's run (states never decrease along t: one run, one writer each)
        for (int t = tid; t < tb; t += NT) {
            const int q = stt[t];
            if (q & 1) {
                if (t == 0 || stt[t - 1] != q) sp[2 * (p0 + (q >> 1))] = t;
                if (t == tb - 1 || stt[t + 1] != q) sp[2 * (p0 + (q >> 1)) + 1] = t;
            }
        }
    }
    __syncthreads();
    for (int p = tid; p < P; p += NT) {   // thread = token
        const int j = p - p0;
        float acc = 0.f;
        if (aligned && j >= 0 && j < L) {
            const int f = sp[2 * p], l = sp[2 * p + 1];
            if (f >= 0) {   // t ascending, single adds
                const int c = cl_clamp_tok(tokens[(long)b * P + p], C);
                for (int t = f; t <= l; ++t) acc += lrow[(long)t * C + c];
            } else {
                sp[2 * p + 1] = -1;
            }
        }
        tl[p] = acc;
    }
    if (ft)
        for (int t = tid; t < T; t += NT) {
            int v = -1;
            if (aligned && t < tb) {
                const int q = stt[t];
                if (q & 1) v = p0 + (q >> 1);
            }
            ft[t] = v;
        }
}

}  // namespace

size_t ctc_align_long_ws_bytes(int B, int T, int P) {
    if (B < 1 || T < 1 || T > CL_MAXT || P < 1 || P > CL_MAXP) return 0;
    return (size_t)B * cl_row_bytes(T, P);
}

hipError_t launch_ctc_align_long(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P,
                                 int C, int* spans, float* tok_logp, int* frame_tok, float* score, void* ws, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (T < 1 || T > CL_MAXT || P < 1 || P > CL_MAXP || C < 2 || C > CL_MAXC || !ws) return hipErrorInvalidValue;
    const int W = cl_words(P);
    int nt = (W + 63) / 64 * 64;
    nt = nt < CL_MINNT ? CL_MINNT : nt;   // (>= C: the first C threads load the emission rows)
    ProfScope ps(st, "ctc_align_long", 6.0 * B * T * (2.0 * P + 1), 4.0 * B * T * C + 16.0 * B * T * W);
    hipLaunchKernelGGL(ctc_align_long_kernel, dim3(B), dim3(nt), 0, st, logp, t_len, tokens, p0, p1, T, P, C, W, cl_row_bytes(T, P),
                       cl_off_state(T, P), spans, tok_logp, frame_tok, score, static_cast<char*>(ws));
    return hipGetLastError();
}
