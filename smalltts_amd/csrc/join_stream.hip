// Running join (DESIGN '8h. Streamed long-form'), gfx950: the joined stream of a long text handed out batch by batch.
// The contract is written out in include/smalltts_hip.h (smtts_join_stream); this file is the two kernels and the entry.
//
// join_stream_kernel: blockIdx.y = row (piece) b, blockIdx.x = a tile of JS_TILE consecutive samples of what the piece emits: its
// gap (if it has one) and then its window.  Nobody hands the workgroup its offset: it reads the state slot (pos, k) and the windows
// of the rows in front of it from the seg table (at most 1023 of them, four per thread, summed through LDS: integers, so the order of
// the sum cannot matter) and places itself.  With m = the non-empty rows in front of b in this call and s = the samples of their
// windows, the gaps in front of the (m + 1)-th non-empty piece, its own included, number m + 1 where k > 0 and m otherwise; an empty
// piece sits where the last non-empty one ended.  The gap is written as zeros by the piece behind it, so the chunk needs no fill
// launch and nothing behind its length is touched.  The sample arithmetic is stitch_kernel's (kernels.hip), one fp32 multiply per
// step, so that the chunks' concatenation is smtts_stitch_seg's buffer bit for bit.
//
// join_advance_kernel (a second launch behind the first, so that no workgroup of the first can see the slot half updated): one
// workgroup sums ALL rows the same way, then one thread writes rec, the delivery row and the slot: every load of the slot precedes
// the store to it.
//
// Bandwidth-bound and tiny next to the codec: plain C++, no atomics, nothing scheduling-dependent.
#include "../../include/smalltts_hip.h"

#include <cstdint>

#include "capi_handle.hpp"
#include "prof.hpp"

namespace {

constexpr int JS_THREADS = 256;
constexpr int JS_PER = 4;                          // samples per thread
constexpr int JS_TILE = JS_THREADS * JS_PER;       // samples per workgroup
constexpr int JS_MAX_B = 1024;                     // JS_PER table rows per thread cover every row in front

struct JsWin { long s0, n; };

// smtts_stitch_seg's clamp into the row (a negative n is an empty window)
__device__ __forceinline__ JsWin js_win(const int64_t* __restrict__ seg, int b, long row_stride) {
    JsWin w;
    const long a = (long)seg[2 * b], n = (long)seg[2 * b + 1];
    w.s0 = a < 0 ? 0 : a > row_stride ? row_stride : a;
    w.n = n < row_stride - w.s0 ? n : row_stride - w.s0;
    if (w.n < 0) w.n = 0;
    return w;
}

// over the rows [0, rows): (samples of their windows, how many are non-empty), the same pair in every thread.  Two barriers.
__device__ __forceinline__ void js_sum(const int64_t* __restrict__ seg, int rows, long row_stride, long* lds_n, int* lds_c, long& sum,
                                       int& cnt) {
    long s = 0;
    int c = 0;
    for (int r = threadIdx.x; r < rows; r += JS_THREADS) {
        const long n = js_win(seg, r, row_stride).n;
        s += n;
        c += n > 0;
    }
    lds_n[threadIdx.x] = s;
    lds_c[threadIdx.x] = c;
    __syncthreads();
    for (int w = JS_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            lds_n[threadIdx.x] += lds_n[threadIdx.x + w];
            lds_c[threadIdx.x] += lds_c[threadIdx.x + w];
        }
        __syncthreads();
    }
    sum = lds_n[0];
    cnt = lds_c[0];
}

// gaps in front of the first m non-empty pieces of this call, on a stream that held k non-empty pieces before it
__device__ __forceinline__ long js_gaps(long k, int m) { return k > 0 ? m : (m > 0 ? m - 1 : 0); }

__device__ __forceinline__ void js_put(float* y, float v) { *y = v; }
__device__ __forceinline__ void js_put(int16_t* y, float v) { *y = (int16_t)__float2int_rn(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f); }

template <class T>
__global__ __launch_bounds__(JS_THREADS) void join_stream_kernel(const float* __restrict__ audio, long row_stride,
                                                                 const int64_t* __restrict__ seg, const float* __restrict__ gain,
                                                                 const float* __restrict__ fade, int F, long gap,
                                                                 const int64_t* __restrict__ state, T* __restrict__ chunk, long chunk_cap,
                                                                 int64_t* __restrict__ off) {
    __shared__ long lds_n[JS_THREADS];
    __shared__ int lds_c[JS_THREADS];
    const int b = blockIdx.y;
    const JsWin w = js_win(seg, b, row_stride);
    const long t0 = (long)blockIdx.x * JS_TILE;          // this tile's first sample, counted from the start of the piece's gap
    if (blockIdx.x != 0 && t0 >= gap + w.n) return;      // the same for every thread; tile 0 stays: it owns off[b]
    const long pos0 = (long)state[0], k0 = (long)state[1];
    long s_front;
    int m_front;
    js_sum(seg, b, row_stride, lds_n, lds_c, s_front, m_front);
    const bool has_gap = w.n > 0 && (k0 > 0 || m_front > 0);
    const long g_b = has_gap ? gap : 0;
    // relative to the chunk: where the piece's window starts
    const long rel = s_front + gap * js_gaps(k0, m_front) + g_b;
    if (blockIdx.x == 0 && threadIdx.x == 0) off[b] = (int64_t)(pos0 + rel);
    if (w.n == 0) return;
    const long Fb = F < w.n / 2 ? F : w.n / 2;
    const float* const xr = audio + (long)b * row_stride + w.s0;
    const bool has_gain = gain != nullptr;
    const float gn = has_gain ? gain[b] : 1.0f;
    const long e0 = rel - g_b;                           // chunk index of the piece's first emitted sample (its gap's, if any)
#pragma unroll
    for (int j = 0; j < JS_PER; ++j) {
        const long t = t0 + (long)j * JS_THREADS + threadIdx.x;   // lanes along the samples: coalesced
        if (t >= g_b + w.n) continue;
        const long c = e0 + t;
        if (c >= chunk_cap) continue;                    // dropped; rec still carries the untruncated position
        float v = 0.0f;
        if (t >= g_b) {
            const long i = t - g_b;
            v = xr[i];
            if (has_gain) v = v * gn;
            if (i < Fb) v = v * fade[i];
            else if (i >= w.n - Fb) v = v * fade[w.n - 1 - i];
        }
        js_put(chunk + c, v);
    }
}

__global__ __launch_bounds__(JS_THREADS) void join_advance_kernel(const int64_t* __restrict__ seg, int B, long row_stride, long gap, int last,
                                                                  int64_t* state, int64_t* __restrict__ rec, int64_t* __restrict__ dtable,
                                                                  long slot) {
    __shared__ long lds_n[JS_THREADS];
    __shared__ int lds_c[JS_THREADS];
    const long pos0 = (long)state[0], k0 = (long)state[1];
    long s_all;
    int m_all;
    js_sum(seg, B, row_stride, lds_n, lds_c, s_all, m_all);   // its barriers stand between the loads of the slot and the stores
    if (threadIdx.x != 0) return;
    const long pos1 = pos0 + s_all + gap * js_gaps(k0, m_all);
    rec[0] = pos0; rec[1] = pos1; rec[2] = k0; rec[3] = k0 + m_all;
    if (dtable) { dtable[0] = slot; dtable[1] = pos0; dtable[2] = pos1 - pos0; dtable[3] = last != 0; }
    state[0] = pos1;
    state[1] = k0 + m_all;
}

}  // namespace

extern "C" {

int smtts_join_stream(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* seg, const float* gain,
                      const float* fade, int F, int64_t gap, int last, int64_t* state, void* chunk, int64_t chunk_cap, int pcm16,
                      int64_t* off, int64_t* rec, int64_t* dtable, int64_t slot) { NULLCHK;
    if (B < 1 || B > JS_MAX_B) return E.fail("smtts_join_stream: B must be in [1, 1024]");
    if (row_stride < 1 || row_stride > (int64_t)1 << 40) return E.fail("smtts_join_stream: row_stride must be in [1, 2^40]");
    if (!audio || !seg || !off || !rec || !chunk || !state) return E.fail("smtts_join_stream: a required pointer is NULL");
    if (reinterpret_cast<uintptr_t>(state) & 15) return E.fail("smtts_join_stream: the state slot must be 16-byte aligned");
    if (gap < 0 || gap > (int64_t)1 << 31) return E.fail("smtts_join_stream: gap must be in [0, 2^31]");
    if (F < 0 || (F > 0 && !fade)) return E.fail("smtts_join_stream: F must be >= 0, and F > 0 needs a fade table");
    if (chunk_cap < 1) return E.fail("smtts_join_stream: chunk_cap must be at least 1");
    hipStream_t st = ST(stream);
    const long tiles = (long)((row_stride + gap + JS_TILE - 1) / JS_TILE);   // <= (2^40 + 2^31) / 1024 + 1: fits a grid dimension
    {
        ProfScope ps(st, "join_stream", (gain ? 2.0 : 1.0) * B * (double)row_stride, (4.0 + (pcm16 ? 2.0 : 4.0)) * B * (double)row_stride);
        if (pcm16)
            hipLaunchKernelGGL(join_stream_kernel<int16_t>, dim3((unsigned)tiles, (unsigned)B), dim3(JS_THREADS), 0, st, audio, (long)row_stride,
                               seg, gain, fade, F, (long)gap, state, static_cast<int16_t*>(chunk), (long)chunk_cap, off);
        else
            hipLaunchKernelGGL(join_stream_kernel<float>, dim3((unsigned)tiles, (unsigned)B), dim3(JS_THREADS), 0, st, audio, (long)row_stride,
                               seg, gain, fade, F, (long)gap, state, static_cast<float*>(chunk), (long)chunk_cap, off);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_join_stream");
    }
    {
        ProfScope ps(st, "join_advance", 0.0, 16.0 * B + 96.0);
        hipLaunchKernelGGL(join_advance_kernel, dim3(1), dim3(JS_THREADS), 0, st, seg, B, (long)row_stride, (long)gap, last, state, rec, dtable,
                           (long)slot);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_join_stream");
    }
    return 0;
}

}  // extern "C"
