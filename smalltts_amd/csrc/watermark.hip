// Watermark (DESIGN '8k. Watermark'), gfx950: a keyed, additive spread-spectrum mark on the 24 kHz stream and its detector.
// The contract is written out in include/smalltts_hip.h (smtts_watermark, smtts_watermark_detect); this file is the kernels and the
// two entries.  Plain C++, no atomics, nothing scheduling-dependent.
//
// wm_embed_kernel: blockIdx.y = row, blockIdx.x = a tile of WM_TILE consecutive samples of the row's chunk, one thread per sample.
// The tile's samples lie in at most WM_TILE / 64 + 1 blocks of the absolute stream; their amplitudes follow the envelopes of the
// blocks in front, so the workgroup stages the stream from the start of the first of those (64 .. 127 samples in front of the tile)
// in LDS, from the chunk or the slot as deliver_kernel does.  One thread per envelope runs the 64-step chain, three threads of
// another wave run the Philox calls that cover the tile's chips (one call per 128 samples), a barrier, one thread per sample marks.
//
// wm_carry_kernel (a second launch behind the first, so that no workgroup of the first can see a slot half updated): one workgroup
// per row gathers the stream's last 127 UNMARKED samples into LDS, passes a barrier and stores them.
//
// wm_u_kernel: blockIdx.y = row, blockIdx.x = a tile of WD_TILE samples, WD_THREADS threads with four samples each.  y^2 and d2^2 of
// the tile's neighbourhood are staged in LDS once, every sample then runs its two 64-term chains out of LDS (consecutive lanes read
// consecutive words: no bank conflict).  The tile's sum of u^2 leaves through a fixed LDS tree.
//
// wm_corr_kernel, the hot one (len * n_off sign-adds): blockIdx.y = row, blockIdx.x = a tile of 256 offsets, one thread per offset.
// Per tile of 1024 samples the workgroup stages u (every lane then reads the same address: a broadcast) and the 1024 + 256 chips the
// tile needs as bits (13 Philox calls); a thread slides a 64-bit window over the bits in registers and flips u's sign bit by XOR.
//
// wm_best_kernel: one workgroup per row: den's second tree, the argmax over T (lowest offset on ties), z.
#include "../../include/smalltts_hip.h"

#include <cmath>
#include <cstdint>

#include "capi_handle.hpp"
#include "philox.hpp"
#include "prof.hpp"

// Every fp32 operation of this unit is the one written: hipcc would contract a * b + c into an fma by default, and its __fadd_rn /
// __fmul_rn are the plain operators (its __fsqrt_rn the native approximation), so they do not keep a product and a sum apart.  The
// pragma does; sqrtf and / are the correctly rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma clang fp contract(off)

namespace {

constexpr int WM_TILE = 256;                    // samples (= threads) per embedding workgroup
constexpr int WM_HIST = 127;                    // samples a slot carries
constexpr int WM_WIN = WM_TILE + 128;           // the staged window: at most 127 samples in front of the tile
constexpr int WM_ENV = WM_TILE / 64 + 1;        // envelopes a tile can need
constexpr int WM_PHX = WM_TILE / 128 + 1;       // Philox calls a tile can need
constexpr uint32_t WM_STREAM = 0x574D4B31u;     // 'WMK1'

constexpr int WD_TILE = 1024;                   // samples per detector tile
constexpr int WD_THREADS = 256;
constexpr int WD_SQ = WD_TILE + 64;             // y^2 over [t0 - 96, t0 + 1023 - 33], d2^2 over [t0 - 32, t0 + 1023 + 31]: 1087 each
constexpr int WD_OFFS = 256;                    // offsets (= threads) per correlation workgroup
constexpr int WD_GROUPS = 13;                   // Philox calls per correlation tile: (127 + 255 + 1023 + 64) / 128 + 1
constexpr float WD_EPS = 1e-8f;

struct WmRow { long slot, nb, len; };

__device__ __forceinline__ WmRow wm_row(const int64_t* __restrict__ table, int b, long row_stride, long n_slots, bool pooled) {
    WmRow r;
    r.slot = (long)table[4 * b + 0];
    r.nb = (long)table[4 * b + 1];
    r.len = (long)table[4 * b + 2];
    r.slot = r.slot < 0 ? 0 : r.slot >= n_slots ? n_slots - 1 : r.slot;   // the table lives on the device: clamped, never followed
    r.len = r.len < 0 ? 0 : r.len > row_stride ? row_stride : r.len;
    r.nb = r.nb < 0 ? 0 : r.nb > (1L << 50) ? (1L << 50) : r.nb;
    if (!pooled) r.nb = 0;                                                // "every row starts here"
    return r;
}

// the four words that hold the chips of the samples [128 g, 128 g + 128)
__device__ __forceinline__ void wm_chip_words(long g, uint64_t key, uint32_t w[4]) {
    w[0] = (uint32_t)g; w[1] = (uint32_t)((uint64_t)g >> 32); w[2] = WM_STREAM; w[3] = 0u;
    philox4x32_10(w, (uint32_t)key, (uint32_t)(key >> 32));
}

__global__ __launch_bounds__(WM_TILE) void wm_embed_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ table,
                                                           uint64_t key, float strength, const char* __restrict__ pool, long n_slots,
                                                           float* __restrict__ out) {
    __shared__ float win[WM_WIN];
    __shared__ float amp[WM_ENV];
    __shared__ uint32_t bits[4 * WM_PHX];
    const int b = blockIdx.y;
    const WmRow r = wm_row(table, b, row_stride, n_slots, pool != nullptr);
    const long c0 = (long)blockIdx.x * WM_TILE;          // this tile's first sample in the chunk
    if (c0 >= r.len) return;                             // the same for every thread of the workgroup
    const int tn = r.len - c0 < WM_TILE ? (int)(r.len - c0) : WM_TILE;
    const long i0 = r.nb + c0;                           // ... and in the stream
    const long k_lo = i0 >> 6, k_hi = (i0 + tn - 1) >> 6;
    const long w0 = (k_lo - 1) * 64;                     // stream index of the window's first sample (-64 in front of block 0)
    const int wn = (int)(i0 + tn - w0);                  // <= 127 + WM_TILE
    const float* const hist = pool ? reinterpret_cast<const float*>(pool + r.slot * 512) : nullptr;
    const float* const row = audio + (long)b * row_stride;
    for (int i = threadIdx.x; i < wn; i += WM_TILE) {
        const long s = w0 + i;
        float v = 0.0f;
        if (s >= r.nb) v = row[s - r.nb];
        else if (hist && s >= 0 && s >= r.nb - WM_HIST) v = hist[WM_HIST + (s - r.nb)];
        win[i] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < WM_ENV && k_lo + t <= k_hi) {                // A[k_lo + t] from block k_lo + t - 1 = win[64 t .. 64 t + 64)
        float a = 0.0f;
        if (k_lo + t > 0) {
            float acc = 0.0f;
            for (int j = 0; j < 64; ++j) {
                const float x = win[64 * t + j];
                acc = acc + x * x;
            }
            a = strength * sqrtf(acc * 0.015625f);
        }
        amp[t] = a;
    } else if (t >= 64 && t < 64 + WM_PHX) {
        uint32_t w[4];
        wm_chip_words((i0 >> 7) + (t - 64), key, w);
        for (int q = 0; q < 4; ++q) bits[4 * (t - 64) + q] = w[q];
    }
    __syncthreads();
    if (t >= tn) return;
    const long i = i0 + t;
    const float a = amp[(int)((i >> 6) - k_lo)];
    const uint32_t word = bits[4 * (int)((i >> 7) - (i0 >> 7)) + (int)((i >> 5) & 3)];
    const float x = win[(int)(i - w0)];
    out[(long)b * row_stride + c0 + t] = (word >> (i & 31)) & 1u ? x + a : x - a;
}

__global__ __launch_bounds__(128) void wm_carry_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ table,
                                                       char* pool, long n_slots) {
    __shared__ float keep[128];
    const int b = blockIdx.x;
    const WmRow r = wm_row(table, b, row_stride, n_slots, true);
    float* const hist = reinterpret_cast<float*>(pool + r.slot * 512);
    const float* const row = audio + (long)b * row_stride;
    const int j = threadIdx.x;
    // new[j] = stream sample n - 127 + j: from the chunk where that index is >= n_before, the old slot moved up by len otherwise
    if (j < WM_HIST) {
        const long c = r.len - WM_HIST + j;
        keep[j] = c >= 0 ? row[c] : hist[j + r.len];
    }
    __syncthreads();
    if (j < WM_HIST) hist[j] = keep[j];
}

__device__ __forceinline__ long wd_len(const int64_t* __restrict__ len, int b, long row_stride) {
    const long n = (long)len[b];
    return n < 0 ? 0 : n > row_stride ? row_stride : n;
}

__global__ __launch_bounds__(WD_THREADS) void wm_u_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ len,
                                                          float* __restrict__ u, float* __restrict__ part, long n_tiles_max) {
    __shared__ float ysq[WD_SQ];
    __shared__ float dsq[WD_SQ];
    __shared__ float red[WD_THREADS];
    const int b = blockIdx.y;
    const long n = wd_len(len, b, row_stride);
    const long t0 = (long)blockIdx.x * WD_TILE;
    if (t0 >= n) return;                                  // the same for every thread; wm_best_kernel reads ceil(n / 1024) partials
    const float* const y = audio + (long)b * row_stride;
    auto Y = [&](long p) { return p >= 0 && p < n ? y[p] : 0.0f; };
    for (int i = threadIdx.x; i < WD_SQ - 1; i += WD_THREADS) {
        const float a = Y(t0 - 96 + i);
        ysq[i] = a * a;
        const long m = t0 - 32 + i;
        float d = 0.0f;
        if (m >= 0 && m < n) d = (Y(m - 1) + Y(m + 1)) - 2.0f * Y(m);
        dsq[i] = d * d;
    }
    __syncthreads();
    float sq = 0.0f;
    for (int q = 0; q < 4; ++q) {
        const int jl = threadIdx.x + WD_THREADS * q;
        const long j = t0 + jl;
        float uj = 0.0f;
        if (j < n) {
            float rs = 0.0f, vs = 0.0f;
            for (int m = 0; m < 64; ++m) { rs += ysq[jl + m]; vs += dsq[jl + m]; }
            const float r = sqrtf(rs * 0.015625f);
            const float v = vs * 0.015625f;
            const float d4 = ((Y(j - 2) + Y(j + 2)) - 4.0f * (Y(j - 1) + Y(j + 1))) + 6.0f * Y(j);
            uj = (d4 * r) / (v + WD_EPS);
            u[(long)b * row_stride + j] = uj;
        }
        sq += uj * uj;
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int s = WD_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)b * n_tiles_max + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(WD_OFFS) void wm_corr_kernel(const float* __restrict__ u, long row_stride, const int64_t* __restrict__ len,
                                                          uint64_t key, long o_lo, int n_off, float* __restrict__ T) {
    __shared__ __attribute__((aligned(16))) float us[WD_TILE];
    __shared__ uint32_t bits[4 * WD_GROUPS];
    const int b = blockIdx.y;
    const long n = wd_len(len, b, row_stride);
    const int oi = blockIdx.x * WD_OFFS + threadIdx.x;   // this thread's offset is o_lo + oi
    const long p_wg = o_lo + (long)blockIdx.x * WD_OFFS; // the workgroup's first offset
    const float* const ur = u + (long)b * row_stride;
    float total = 0.0f;
    for (long t0 = 0; t0 < n; t0 += WD_TILE) {
        const long g0 = (p_wg + t0) >> 7;                // first Philox group of this tile's chips
        const int off = (int)((p_wg + t0) & 127) + threadIdx.x;   // this thread's first chip, as a bit index into `bits`
        __syncthreads();                                 // the previous tile has been read
        for (int i = threadIdx.x; i < WD_TILE; i += WD_OFFS) us[i] = t0 + i < n ? ur[t0 + i] : 0.0f;
        if (threadIdx.x < WD_GROUPS) {
            uint32_t w[4];
            wm_chip_words(g0 + threadIdx.x, key, w);
            for (int q = 0; q < 4; ++q) bits[4 * threadIdx.x + q] = w[q];
        }
        __syncthreads();
        float acc = 0.0f;
        for (int j = 0; j < WD_TILE; j += 32) {
            const int bp = off + j, wi = bp >> 5, sh = bp & 31;   // wi + 1 <= (127 + 255 + 992) / 32 + 1 = 43 < 52
            const uint32_t neg = ~(uint32_t)((((uint64_t)bits[wi + 1] << 32) | bits[wi]) >> sh);   // a set bit: chip -1
#pragma unroll
            for (int jj = 0; jj < 32; jj += 4) {
                const float4 x = *reinterpret_cast<const float4*>(us + j + jj);
                acc = acc + __uint_as_float(__float_as_uint(x.x) ^ (((neg >> (jj + 0)) & 1u) << 31));
                acc = acc + __uint_as_float(__float_as_uint(x.y) ^ (((neg >> (jj + 1)) & 1u) << 31));
                acc = acc + __uint_as_float(__float_as_uint(x.z) ^ (((neg >> (jj + 2)) & 1u) << 31));
                acc = acc + __uint_as_float(__float_as_uint(x.w) ^ (((neg >> (jj + 3)) & 1u) << 31));
            }
        }
        total = total + acc;
    }
    if (oi < n_off) T[(long)b * n_off + oi] = total;
}

__global__ __launch_bounds__(WD_THREADS) void wm_best_kernel(const float* __restrict__ part, long n_tiles_max, long row_stride,
                                                             const int64_t* __restrict__ len, const float* __restrict__ T, long o_lo,
                                                             int n_off, float* __restrict__ den, int64_t* __restrict__ best_off,
                                                             float* __restrict__ best_z) {
    __shared__ float red[WD_THREADS];
    __shared__ int idx[WD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const long n = wd_len(len, b, row_stride);
    const long nt = (n + WD_TILE - 1) / WD_TILE;
    float s = 0.0f;
    for (long i = t; i < nt; i += WD_THREADS) s += part[(long)b * n_tiles_max + i];
    red[t] = s;
    __syncthreads();
    for (int k = WD_THREADS / 2; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    const float d = red[0];
    __syncthreads();
    // argmax, the lowest index on ties: a thread's own indices ascend, the tree keeps the lower index of equal values
    const float* const Tr = T + (long)b * n_off;
    float best = 0.0f;
    int bi = -1;
    for (int i = t; i < n_off; i += WD_THREADS) {
        const float v = Tr[i];
        if (bi < 0 || v > best) { best = v; bi = i; }
    }
    red[t] = best;
    idx[t] = bi;
    __syncthreads();
    for (int k = WD_THREADS / 2; k > 0; k >>= 1) {
        if (t < k) {
            const int oi = idx[t + k];
            const float ov = red[t + k];
            if (oi >= 0 && (idx[t] < 0 || ov > red[t] || (ov == red[t] && oi < idx[t]))) { red[t] = ov; idx[t] = oi; }
        }
        __syncthreads();
    }
    if (t == 0) {
        den[b] = d;
        best_off[b] = (int64_t)(o_lo + idx[0]);
        best_z[b] = d == 0.0f ? 0.0f : red[0] / sqrtf(d);
    }
}

size_t wd_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

size_t smtts_watermark_state_bytes(smtts_handle h) { NULLCHK0;
    return 512;
}

int smtts_watermark(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* table, uint64_t key,
                    float strength, void* state_pool, int64_t n_slots, float* out) { NULLCHK;
    if (B < 1 || B > 65535) return E.fail("smtts_watermark: B must be in [1, 65535]");
    if (row_stride < 1 || row_stride > (int64_t)1 << 40) return E.fail("smtts_watermark: row_stride must be in [1, 2^40]");
    if (!audio || !table || !out) return E.fail("smtts_watermark: a required pointer is NULL");
    if (!(strength >= 0.0f) || !(strength <= 1.0f)) return E.fail("smtts_watermark: strength must be finite and in [0, 1]");
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(audio), o = reinterpret_cast<uintptr_t>(out);
        const uintptr_t bytes = (uintptr_t)B * (uintptr_t)row_stride * sizeof(float);
        if (a < o + bytes && o < a + bytes) return E.fail("smtts_watermark: audio and out overlap (in place is a race on the block in front)");
    }
    if (state_pool) {
        if (n_slots < 1) return E.fail("smtts_watermark: the state pool has no slots");
        if (reinterpret_cast<uintptr_t>(state_pool) & 15) return E.fail("smtts_watermark: the state pool must be 16-byte aligned");
    }
    const long tiles = (long)((row_stride + WM_TILE - 1) / WM_TILE);
    if (tiles > 0x7fffffffL) return E.fail("smtts_watermark: row_stride too large for one launch");
    hipStream_t st = ST(stream);
    {
        ProfScope ps(st, "watermark", 130.0 * B * (double)row_stride / 64, 8.0 * B * (double)row_stride);
        hipLaunchKernelGGL(wm_embed_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(WM_TILE), 0, st, audio, (long)row_stride, table, key,
                           strength, static_cast<const char*>(state_pool), (long)n_slots, out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_watermark");
    }
    if (state_pool) {
        ProfScope ps(st, "watermark_carry", 0.0, 8.0 * B * WM_HIST);
        hipLaunchKernelGGL(wm_carry_kernel, dim3((unsigned)B), dim3(128), 0, st, audio, (long)row_stride, table,
                           static_cast<char*>(state_pool), (long)n_slots);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_watermark");
    }
    return 0;
}

size_t smtts_watermark_detect_workspace_bytes(smtts_handle h, int B, int64_t row_stride) { NULLCHK0;
    if (B < 1 || B > 1024 || row_stride < 1 || row_stride > (int64_t)1 << 40) {
        E.fail("smtts_watermark_detect_workspace_bytes: B must be in [1, 1024], row_stride in [1, 2^40]");
        return 0;
    }
    const size_t n_tiles = (size_t)((row_stride + WD_TILE - 1) / WD_TILE);
    return wd_align((size_t)B * (size_t)row_stride * sizeof(float)) + wd_align((size_t)B * n_tiles * sizeof(float));
}

int smtts_watermark_detect(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, uint64_t key,
                           int64_t o_lo, int n_off, void* ws, size_t ws_bytes, float* u, float* den, float* T, int64_t* best_off,
                           float* best_z) { NULLCHK;
    if (B < 1 || B > 1024) return E.fail("smtts_watermark_detect: B must be in [1, 1024]");
    if (row_stride < 1 || row_stride > (int64_t)1 << 40) return E.fail("smtts_watermark_detect: row_stride must be in [1, 2^40]");
    if (!audio || !len || !ws || !den || !T || !best_off || !best_z) return E.fail("smtts_watermark_detect: a required pointer is NULL");
    if (o_lo < 0 || o_lo > (int64_t)1 << 40) return E.fail("smtts_watermark_detect: o_lo must be in [0, 2^40]");
    if (n_off < 1 || n_off > 65536) return E.fail("smtts_watermark_detect: n_off must be in [1, 65536]");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return E.fail("smtts_watermark_detect: the workspace must be 256-byte aligned");
    const long n_tiles = (long)((row_stride + WD_TILE - 1) / WD_TILE);
    if (n_tiles > 0x7fffffffL) return E.fail("smtts_watermark_detect: row_stride too large for one launch");
    const size_t u_bytes = wd_align((size_t)B * (size_t)row_stride * sizeof(float));
    if (ws_bytes < u_bytes + wd_align((size_t)B * (size_t)n_tiles * sizeof(float)))
        return E.fail("smtts_watermark_detect: workspace smaller than smtts_watermark_detect_workspace_bytes");
    float* const uu = u ? u : static_cast<float*>(ws);
    float* const part = reinterpret_cast<float*>(static_cast<char*>(ws) + u_bytes);
    hipStream_t st = ST(stream);
    {
        ProfScope ps(st, "watermark_u", 400.0 * B * (double)row_stride, 8.0 * B * (double)row_stride);
        hipLaunchKernelGGL(wm_u_kernel, dim3((unsigned)n_tiles, (unsigned)B), dim3(WD_THREADS), 0, st, audio, (long)row_stride, len, uu, part,
                           n_tiles);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_watermark_detect");
    }
    {
        ProfScope ps(st, "watermark_corr", 1.0 * B * (double)row_stride * n_off, 4.0 * B * ((double)row_stride * ((n_off + 255) / 256) + n_off));
        hipLaunchKernelGGL(wm_corr_kernel, dim3((unsigned)((n_off + WD_OFFS - 1) / WD_OFFS), (unsigned)B), dim3(WD_OFFS), 0, st, uu,
                           (long)row_stride, len, key, (long)o_lo, n_off, T);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_watermark_detect");
    }
    {
        ProfScope ps(st, "watermark_best", 0.0, 4.0 * B * ((double)n_tiles + n_off));
        hipLaunchKernelGGL(wm_best_kernel, dim3((unsigned)B), dim3(WD_THREADS), 0, st, part, n_tiles, (long)row_stride, len, T, (long)o_lo,
                           n_off, den, best_off, best_z);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_watermark_detect");
    }
    return 0;
}

}  // extern "C"
