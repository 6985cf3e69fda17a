// Retiming (DESIGN '8n. Retiming'), gfx950: WSOLA time-scale modification of the 24 kHz waveform onto a table of (source, target)
// anchors.  The contract is written out in include/smalltts_hip.h (smtts_retime); this file is the kernel and the entry.
// Plain C++, no atomics, nothing scheduling-dependent.
//
// retime_kernel: one workgroup of RT_THREADS threads per row walks the row's segments in order: segment k's search needs q_{k-1}.
// What a segment reads is known without the chain: every q_k lies within D of p_k = M(kH) (segment 0: q = p; a continuation:
// |c - p| <= D; a search: q = p + lag), so the REGION x[p_k - D, p_k + D + 2H) holds segment k's candidates, the samples it copies
// or cross-fades from q_k, AND the next segment's template x[q_k + H, q_k + 2H).  The regions of segments k + 1 and k + 2 are on
// their way from global memory into registers while segment k is worked on (a copy segment is shorter than one memory latency),
// and a region is stored to LDS at the top of its own iteration; three LDS regions rotate
// (the one being filled, the current one, the previous one), so that one barrier per segment suffices.  Samples outside [0, n) are
// written into the region as +0.0: nothing behind n is loaded, and no later stage needs a bounds check.
// A search: the template is first copied to a 16-byte aligned LDS array, so that it is read as ds_read_b128 from one address in all
// lanes (a broadcast); lags go across the lanes, candidates are read at stride 1 (consecutive lanes, consecutive banks).  The argmax
// with its tie rule is a wave butterfly and one LDS step over the four waves.  A NaN score is replaced by -inf before it is compared,
// so the rule is a strict total order on (score, lag) and every lane of a wave ends with the same winner; the workgroup's winner is
// uniform in any case, because every thread repeats the same compare of the four wave results out of LDS.  The anchor index only
// moves forward; all of the map's arithmetic is uniform across the workgroup.
#include "../../include/smalltts_hip.h"

#include <climits>
#include <cmath>
#include <cstdint>

#include "capi_handle.hpp"
#include "prof.hpp"

// The cross-fade is three separately rounded fp32 operations.  hipcc contracts a * b + c into an fma by default, and its __fmul_rn /
// __fadd_rn do not prevent that: they are the plain operators compiled under the header's contraction mode, so once inlined their
// product and sum fuse like any other.  The pragma below keeps them apart for the plain operators written in this file, which is how
// the cross-fade is written.  It governs EVERY a * b + c of this file, also one added later: what wants an fma asks for fmaf by name,
// as the dot products do.
#pragma clang fp contract(off)

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_MAX_HOP = 512, RT_MAX_DELTA = 512;
constexpr int RT_REGION = 2 * RT_MAX_DELTA + 2 * RT_MAX_HOP;   // floats of one region: 2 D + 2 H
constexpr int RT_PRE = RT_REGION / RT_THREADS;                 // floats of the next region a thread holds in registers
constexpr int RT_NONE = INT_MIN;                               // "no candidate yet"

__device__ __forceinline__ long rt_clamp(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }

// The map M of the header, evaluated at increasing t.  Every table entry is clamped as it is loaded (src into [0, row_stride], dst
// into [0, out_stride]): the products below then fit int64 whatever the table holds.
struct RtMap {
    const int64_t* __restrict__ a;   // the row's (src, dst) pairs
    int m, j;                        // anchors in use, the current segment's first anchor (never moves back)
    long n, row_stride, out_stride;

    __device__ __forceinline__ long src(int i) const { return rt_clamp((long)a[2 * i], 0, row_stride); }
    __device__ __forceinline__ long dst(int i) const { return rt_clamp((long)a[2 * i + 1], 0, out_stride); }

    __device__ long at(long t) {
        long d0 = 0, d1 = 0;
        while (j + 1 < m) {                                   // at most m steps over the whole row
            d0 = dst(j);
            d1 = dst(j + 1);
            if (d1 > d0 && t >= d0 && t < d1) break;          // a segment that does not increase is skipped
            ++j;
        }
        long r;
        if (j + 1 < m) {
            const long num = (t - d0) * (src(j + 1) - src(j)), den = d1 - d0;   // |num| < 2^62, den > 0
            long fl = num / den;
            if (num % den < 0) --fl;                          // floor, as Python's //
            r = src(j) + fl;
        } else {
            r = src(m - 1) + (t - dst(m - 1));
        }
        return rt_clamp(r, 0, n);
    }
};

// does (s1, d1) beat (s0, d0)?  The larger score; on equal scores the smaller |lag|, then the negative lag.  No score is NaN here.
__device__ __forceinline__ bool rt_better(float s1, int d1, float s0, int d0) {
    if (d1 == RT_NONE) return false;
    if (d0 == RT_NONE) return true;
    if (s1 > s0) return true;
    if (!(s1 == s0)) return false;
    const int a1 = d1 < 0 ? -d1 : d1, a0 = d0 < 0 ? -d0 : d0;
    return a1 < a0 || (a1 == a0 && d1 < d0);
}

__global__ __launch_bounds__(RT_THREADS) void retime_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ len,
                                                            const int64_t* __restrict__ anchors, const int64_t* __restrict__ n_anchor,
                                                            int A, const float* __restrict__ win, int H, int D, float* __restrict__ out,
                                                            long out_stride, int64_t* __restrict__ q, long Kmax) {
    __shared__ __attribute__((aligned(16))) float region[3][RT_REGION];
    __shared__ __attribute__((aligned(16))) float tmpl[RT_MAX_HOP];
    __shared__ float w[2 * RT_MAX_HOP];
    __shared__ float red_s[RT_WAVES];
    __shared__ int red_d[RT_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long n = rt_clamp((long)len[b], 0, row_stride);
    const int m = (int)rt_clamp((long)n_anchor[b], 0, A);
    if (m < 2) return;                                        // the same for every thread of the workgroup, like every branch on k below
    RtMap M{anchors + (long)b * A * 2, m, 0, n, row_stride, out_stride};
    const long out_len = M.dst(m - 1);
    if (out_len == 0) return;
    const long K = (out_len + H - 1) / H;
    const float* const x = audio + (long)b * row_stride;
    float* const y = out + (long)b * out_stride;
    int64_t* const qr = q ? q + (long)b * Kmax : nullptr;
    const int R = 2 * D + 2 * H;
    for (int i = tid; i < 2 * H; i += RT_THREADS) w[i] = win[i];   // visible behind the first barrier below

    float pre[RT_PRE], pre2[RT_PRE] = {};                     // the regions of the next segment and of the one behind it
    auto fetch = [&](long p0, float (&dst)[RT_PRE]) {         // x[p0 - D, p0 + D + 2H) -> registers, +0.0 outside [0, n)
#pragma unroll
        for (int j = 0; j < RT_PRE; ++j) {
            const int i = tid + j * RT_THREADS;
            const long s = p0 - D + i;
            dst[j] = (i < R && s >= 0 && s < n) ? x[s] : 0.0f;
        }
    };
    long p = M.at(0), p_prev = 0, q_prev = 0;
    long p_next = K > 1 ? M.at(H) : 0;
    fetch(p, pre);
    if (K > 1) fetch(p_next, pre2);
    for (long k = 0; k < K; ++k) {
        float* const cur = region[k % 3];
        const float* const prev = region[(k + 2) % 3];
#pragma unroll
        for (int j = 0; j < RT_PRE; ++j) {
            const int i = tid + j * RT_THREADS;
            if (i < R) cur[i] = pre[j];
            pre[j] = pre2[j];
        }
        long p_next2 = 0;
        if (k + 2 < K) {                                      // two regions are on their way while this segment is worked on
            p_next2 = M.at((k + 2) * (long)H);
            fetch(p_next2, pre2);
        }
        const long c = q_prev + H;                            // the natural continuation
        const int t_off = (int)(c - (p_prev - D));            // ... lies in prev at [H, H + 2 D]
        const bool search = k > 0 && (c - p > D || p - c > D);
        if (search)
            for (int i = tid; i < H; i += RT_THREADS) tmpl[i] = prev[t_off + i];
        __syncthreads();
        const long t0 = k * (long)H;
        const int seg_n = out_len - t0 < H ? (int)(out_len - t0) : H;
        long qk;
        if (k == 0) {
            qk = p;
            for (int i = tid; i < seg_n; i += RT_THREADS) y[i] = cur[D + i];
        } else {
            qk = c;
            if (search) {
                float best = 0.0f;
                int bd = RT_NONE;
                for (int l = tid; l <= 2 * D; l += RT_THREADS) {
                    const long pos = p - D + l;
                    if (pos < 0 || pos > n) continue;         // lag 0 always passes: 0 <= p <= n
                    const float* const cd = cur + l;
                    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;   // four chains: the order of the sum is free
                    for (int i = 0; i < H; i += 4) {
                        const float4 t = *reinterpret_cast<const float4*>(tmpl + i);
                        a0 = fmaf(t.x, cd[i], a0);
                        a1 = fmaf(t.y, cd[i + 1], a1);
                        a2 = fmaf(t.z, cd[i + 2], a2);
                        a3 = fmaf(t.w, cd[i + 3], a3);
                    }
                    float acc = (a0 + a1) + (a2 + a3);
                    if (!(acc == acc)) acc = -INFINITY;       // a NaN score (NaN or Inf samples inside len) loses to every number
                    if (rt_better(acc, l - D, best, bd)) { best = acc; bd = l - D; }
                }
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) {
                    const float os = __shfl_xor(best, sh, 64);
                    const int od = __shfl_xor(bd, sh, 64);
                    if (rt_better(os, od, best, bd)) { best = os; bd = od; }
                }
                if ((tid & 63) == 0) { red_s[tid >> 6] = best; red_d[tid >> 6] = bd; }
                __syncthreads();
                best = red_s[0];
                bd = red_d[0];
#pragma unroll
                for (int v = 1; v < RT_WAVES; ++v)
                    if (rt_better(red_s[v], red_d[v], best, bd)) { best = red_s[v]; bd = red_d[v]; }
                if (bd == RT_NONE) bd = 0;                    // unreachable (lag 0 is a candidate); keeps the index in the region anyway
                qk = p + bd;
            }
            if (qk == c) {                                    // the copy: no arithmetic on the sample
                for (int i = tid; i < seg_n; i += RT_THREADS) y[t0 + i] = prev[t_off + i];
            } else {
                const int c_off = (int)(qk - (p - D));        // in [0, 2 D]
                for (int i = tid; i < seg_n; i += RT_THREADS)
                    y[t0 + i] = prev[t_off + i] * w[H + i] + cur[c_off + i] * w[i];   // two products and a sum, each rounded: see the pragma
            }
        }
        if (qr && tid == 0) qr[k] = (int64_t)qk;
        q_prev = qk;
        p_prev = p;
        p = p_next;
        p_next = p_next2;
    }
}

}  // namespace

extern "C" {

int smtts_retime(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, const int64_t* anchors,
                 const int64_t* n_anchor, int A, const float* win, int hop, int delta, float* out, int64_t out_stride, int64_t* q) { NULLCHK;
    if (!audio || !len || !anchors || !n_anchor || !win || !out) return E.fail("smtts_retime: a required pointer is NULL");
    if (B < 1 || B > 1024) return E.fail("smtts_retime: B must be in [1, 1024]");
    if (row_stride < 1 || row_stride > 0x7fffffffLL) return E.fail("smtts_retime: row_stride must be in [1, 2^31 - 1]");
    if (out_stride < 1 || out_stride > 0x7fffffffLL) return E.fail("smtts_retime: out_stride must be in [1, 2^31 - 1]");
    if (A < 2 || A > 65536) return E.fail("smtts_retime: A must be in [2, 65536]");
    if (hop < 16 || hop > RT_MAX_HOP || hop % 4) return E.fail("smtts_retime: hop must be a multiple of 4 in [16, 512]");
    if (delta < 0 || delta > RT_MAX_DELTA) return E.fail("smtts_retime: delta must be in [0, 512]");
    hipStream_t st = ST(stream);
    const long Kmax = (long)((out_stride + hop - 1) / hop);
    ProfScope ps(st, "retime", 2.0 * B * (double)Kmax * hop * (2 * delta + 1), 4.0 * B * ((double)row_stride + (double)out_stride));
    hipLaunchKernelGGL(retime_kernel, dim3((unsigned)B), dim3(RT_THREADS), 0, st, audio, (long)row_stride, len, anchors, n_anchor, A, win, hop,
                       delta, out, (long)out_stride, q, Kmax);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return E.fail_hip(e, "smtts_retime");
    return 0;
}

}  // extern "C"
