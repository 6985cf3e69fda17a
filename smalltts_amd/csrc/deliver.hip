// Delivery (DESIGN '8g. Delivery'), gfx950: audio at the caller's rate and encoding, whole or in chunks that continue each other.
// The contract is written out in include/smalltts_hip.h (smtts_deliver); this file is the two kernels and the entry.
//
// deliver_kernel: blockIdx.y = row, blockIdx.x = a tile of DV_TILE consecutive OUTPUT samples of that row's emission range, one
// thread per sample.  The tile's outputs lie in at most DV_TILE / up + 2 frames, i.e. they read one contiguous window of
// (frames - 1) * down + klen stream samples.  The workgroup first copies that window into LDS with the lanes along it (coalesced;
// sample i of the stream comes from the history slot for i < n_before, from `audio` for n_before <= i < n, and is +0.0f for i < 0
// and for i >= n), and the bank too where up * klen floats fit DV_BANK_LDS bytes (413 floats at 8 kHz; the 147-phase banks of the
// 44.1 kHz family stay in global memory and are served by L2).  Then every thread runs ALL klen taps of its sample in the order
// k = 0 .. klen - 1 as one fmaf chain from +0.0f: a sample is the same sequence of fp32 operations whichever call emits it, which
// is what makes chunked delivery equal whole delivery bit for bit.  The encoders are integer arithmetic on smtts_pcm16's value.
//
// deliver_carry_kernel (a second launch behind the first, so that no workgroup of the first can see a slot half updated): one
// workgroup per row gathers the stream's last H = klen - 1 samples (from the chunk, and from the old slot content where the chunk
// is shorter than H) into LDS, passes a barrier, and stores them: every load of a slot precedes every store to it.
//
// Bandwidth-bound and small next to the codec (8 x 10 s: 1.9 M input samples): plain C++, no atomics, nothing scheduling-dependent.
#include "../../include/smalltts_hip.h"

#include <cstdint>

#include "capi_handle.hpp"
#include "prof.hpp"

namespace {

constexpr int DV_TILE = 256;              // output samples (= threads) per workgroup
constexpr size_t DV_BANK_LDS = 48 << 10;  // a bank up to this many bytes is staged in LDS
constexpr int DV_MAX_KLEN = 8192;         // keeps window + bank and the carry's staging inside LDS

struct DvRow { long slot, nb, len; int last; };

__device__ __forceinline__ DvRow dv_row(const int64_t* __restrict__ table, int b, long row_stride, long n_slots, bool pooled) {
    DvRow r;
    r.slot = (long)table[4 * b + 0];
    r.nb = (long)table[4 * b + 1];
    r.len = (long)table[4 * b + 2];
    r.last = table[4 * b + 3] != 0;
    r.slot = r.slot < 0 ? 0 : r.slot >= n_slots ? n_slots - 1 : r.slot;   // the table lives on the device: clamped, never followed
    r.len = r.len < 0 ? 0 : r.len > row_stride ? row_stride : r.len;
    r.nb = r.nb < 0 ? 0 : r.nb > (1L << 50) ? (1L << 50) : r.nb;          // up * (nb + len) stays inside 64 bits
    if (!pooled) { r.nb = 0; r.last = 1; }   // "every row starts and ends here"
    return r;
}

// smtts_pcm16's arithmetic
__device__ __forceinline__ int dv_pcm16(float x) { return (int)(int16_t)__float2int_rn(fminf(fmaxf(x, -1.0f), 1.0f) * 32767.0f); }

// G.711 as CPython's audioop.lin2ulaw(s, 2) / lin2alaw(s, 2) compute it: the CCITT / Sun g711.c encoders on s >> 2 and s >> 3
__device__ __forceinline__ int dv_seg(int v, int first_end) {   // number of segment ends first_end, 2 first_end + 1, ... below v
    int seg = 0, end = first_end;
#pragma unroll
    for (int i = 0; i < 8; ++i) { seg += v > end; end = 2 * end + 1; }
    return seg;
}
__device__ __forceinline__ int dv_mulaw(int s) {
    int v = s >> 2, mask = 0xFF;
    if (v < 0) { v = -v; mask = 0x7F; }
    if (v > 8159) v = 8159;
    v += 33;
    const int seg = dv_seg(v, 0x3F);
    return seg >= 8 ? (0x7F ^ mask) : ((((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask) & 0xFF);
}
__device__ __forceinline__ int dv_alaw(int s) {
    int v = s >> 3, mask = 0xD5;
    if (v < 0) { v = -v - 1; mask = 0x55; }
    const int seg = dv_seg(v, 0x1F);
    if (seg >= 8) return 0x7F ^ mask;
    return (((seg << 4) | ((v >> (seg < 2 ? 1 : seg)) & 0xF)) ^ mask) & 0xFF;
}

__device__ __forceinline__ void dv_store(void* out, long i, float v, int enc) {
    if (enc == 0) { static_cast<float*>(out)[i] = v; return; }
    const int s = dv_pcm16(v);
    if (enc == 1) static_cast<int16_t*>(out)[i] = (int16_t)s;
    else static_cast<uint8_t*>(out)[i] = (uint8_t)(enc == 2 ? dv_mulaw(s) : dv_alaw(s));
}

// F(m) = max(0, (m - width) / down)
__device__ __forceinline__ long dv_frames(long m, int width, int down) { return m > width ? (m - width) / down : 0; }

// the pass-through rate: a pure encode of the row's len samples
__global__ __launch_bounds__(DV_TILE) void deliver_encode_kernel(const float* __restrict__ audio, long row_stride,
                                                                 const int64_t* __restrict__ table, int enc, void* out, long out_stride) {
    const int b = blockIdx.y;
    const DvRow r = dv_row(table, b, row_stride, 1, false);
    const long j = (long)blockIdx.x * DV_TILE + threadIdx.x;
    if (j >= r.len) return;
    dv_store(out, (long)b * out_stride + j, audio[(long)b * row_stride + j], enc);
}

__global__ __launch_bounds__(DV_TILE) void deliver_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ table,
                                                          const float* __restrict__ bank, int up, int down, int klen, int width,
                                                          const char* __restrict__ pool, long slot_stride, long n_slots, int bank_lds,
                                                          int enc, void* out, long out_stride) {
    extern __shared__ __attribute__((aligned(16))) float dv_lds[];
    const int b = blockIdx.y;
    const DvRow r = dv_row(table, b, row_stride, n_slots, pool != nullptr);
    const long n = r.nb + r.len;
    const long o0 = (long)up * dv_frames(r.nb, width, down);
    const long o1 = r.last ? ((long)up * n + down - 1) / down : (long)up * dv_frames(n, width, down);
    const long ta = o0 + (long)blockIdx.x * DV_TILE;     // this tile's outputs: [ta, tb)
    if (ta >= o1) return;                                // the same for every thread of the workgroup
    const long tb = ta + DV_TILE < o1 ? ta + DV_TILE : o1;
    const long f_lo = ta / up, f_hi = (tb - 1) / up;
    const long w0 = f_lo * down - width;                 // stream index of the window's first sample
    const int wn = (int)(f_hi - f_lo) * down + klen;     // <= (DV_TILE / up + 1) * down + klen: what the launcher sized
    const int H = klen - 1;
    const float* const hist = pool ? reinterpret_cast<const float*>(pool + r.slot * slot_stride) : nullptr;
    const float* const row = audio + (long)b * row_stride;
    for (int i = threadIdx.x; i < wn; i += DV_TILE) {
        const long s = w0 + i;
        float v = 0.0f;
        if (s >= 0 && s < n) {
            if (s >= r.nb) v = row[s - r.nb];
            else if (hist && s >= r.nb - H) v = hist[H + (s - r.nb)];
        }
        dv_lds[i] = v;
    }
    float* const bl = dv_lds + ((wn + 3) & ~3);
    if (bank_lds)
        for (int i = threadIdx.x; i < up * klen; i += DV_TILE) bl[i] = bank[i];
    __syncthreads();
    const long o = ta + threadIdx.x;
    if (o >= tb) return;
    const long f = o / up;
    const int p = (int)(o - f * up);
    const float* const xs = dv_lds + (int)(f - f_lo) * down;
    float acc = 0.0f;
    if (bank_lds) {
        const float* const bp = bl + p * klen;
        for (int k = 0; k < klen; ++k) acc = fmaf(xs[k], bp[k], acc);
    } else {
        const float* const bp = bank + (long)p * klen;
        for (int k = 0; k < klen; ++k) acc = fmaf(xs[k], bp[k], acc);
    }
    dv_store(out, (long)b * out_stride + (o - o0), acc, enc);
}

__global__ __launch_bounds__(256) void deliver_carry_kernel(const float* __restrict__ audio, long row_stride, const int64_t* __restrict__ table,
                                                            int H, char* pool, long slot_stride, long n_slots) {
    extern __shared__ __attribute__((aligned(16))) float dv_lds[];
    const int b = blockIdx.x;
    const DvRow r = dv_row(table, b, row_stride, n_slots, true);
    float* const hist = reinterpret_cast<float*>(pool + r.slot * slot_stride);
    const float* const row = audio + (long)b * row_stride;
    // new[j] = stream sample n - H + j: from the chunk where that index is >= n_before, the old slot moved up by len otherwise
    for (int j = threadIdx.x; j < H; j += 256) {
        const long c = r.len - H + j;
        dv_lds[j] = c >= 0 ? row[c] : hist[j + r.len];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < H; j += 256) hist[j] = dv_lds[j];
}

size_t dv_state_bytes(int klen) { return klen <= 1 ? 0 : (((size_t)(klen - 1) * sizeof(float)) + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

size_t smtts_deliver_state_bytes(smtts_handle h, int klen) { NULLCHK0;
    if (klen > DV_MAX_KLEN) { E.fail("smtts_deliver_state_bytes: klen above 8192"); return 0; }
    return dv_state_bytes(klen);
}

int smtts_deliver(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* table, const float* bank,
                  int up, int down, int klen, int width, void* state_pool, int64_t n_slots, int enc, void* out, int64_t out_stride) { NULLCHK;
    if (B < 1 || B > 65535) return E.fail("smtts_deliver: B must be in [1, 65535]");
    if (row_stride < 1 || row_stride > (int64_t)1 << 40) return E.fail("smtts_deliver: row_stride must be in [1, 2^40]");
    if (!audio || !table || !out) return E.fail("smtts_deliver: a required pointer is NULL");
    if (up < 1 || down < 1 || up > 4096 || down > 4096) return E.fail("smtts_deliver: up and down must be in [1, 4096]");
    if (enc < 0 || enc > 3) return E.fail("smtts_deliver: enc must be 0 (f32), 1 (pcm16), 2 (mu-law) or 3 (A-law)");
    hipStream_t st = ST(stream);
    if (!bank) {
        if (up != 1 || down != 1 || klen != 0 || width != 0 || state_pool)
            return E.fail("smtts_deliver: without a bank only the pass-through rate (up = down = 1, klen = width = 0, no pool)");
        if (out_stride < row_stride) return E.fail("smtts_deliver: out_stride smaller than the largest count");
        const long tiles = ((long)row_stride + DV_TILE - 1) / DV_TILE;
        if (tiles > 0x7fffffffL) return E.fail("smtts_deliver: row_stride too large for one launch");
        ProfScope ps(st, "deliver", 0.0, (4.0 + (enc == 0 ? 4.0 : enc == 1 ? 2.0 : 1.0)) * B * (double)row_stride);
        hipLaunchKernelGGL(deliver_encode_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(DV_TILE), 0, st, audio, (long)row_stride, table,
                           enc, out, (long)out_stride);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : E.fail_hip(e, "smtts_deliver");
    }
    if (width < 0 || klen != 2 * (int64_t)width + down) return E.fail("smtts_deliver: klen must be 2 * width + down");
    if (klen > DV_MAX_KLEN) return E.fail("smtts_deliver: klen above 8192");
    if (state_pool) {
        if (n_slots < 1) return E.fail("smtts_deliver: the state pool has no slots");
        if (reinterpret_cast<uintptr_t>(state_pool) & 15) return E.fail("smtts_deliver: the state pool must be 16-byte aligned");
        if (klen <= 1) return E.fail("smtts_deliver: a bank with klen <= 1 carries no state: pass state_pool = NULL");
    }
    // the largest count a row of row_stride samples can produce: ceil(up (row_stride + width + down - 1) / down) continuing a
    // stream, ceil(up row_stride / down) where every row starts and ends here
    const int64_t span = row_stride + (state_pool ? (int64_t)width + down - 1 : 0);
    const int64_t max_cnt = (up * span + down - 1) / down;
    if (out_stride < max_cnt) return E.fail("smtts_deliver: out_stride smaller than the largest count");
    const long tiles = (long)((max_cnt + DV_TILE - 1) / DV_TILE);
    if (tiles > 0x7fffffffL) return E.fail("smtts_deliver: row_stride too large for one launch");
    const size_t win = ((size_t)((DV_TILE / up + 1) * (long)down + klen) + 3) & ~(size_t)3;
    const size_t bank_bytes = (size_t)up * klen * sizeof(float);
    const int bank_lds = bank_bytes <= DV_BANK_LDS;
    const size_t lds = win * sizeof(float) + (bank_lds ? bank_bytes : 0);
    if (lds > (64 << 10)) return E.fail("smtts_deliver: the window of one tile, (256 / up + 1) * down + klen floats, does not fit 64 KiB of LDS");
    const long slot_stride = (long)dv_state_bytes(klen);
    {
        ProfScope ps(st, "deliver", 2.0 * B * (double)max_cnt * klen, 4.0 * B * ((double)row_stride + (double)max_cnt));
        hipLaunchKernelGGL(deliver_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(DV_TILE), lds, st, audio, (long)row_stride, table, bank,
                           up, down, klen, width, static_cast<const char*>(state_pool), slot_stride, (long)n_slots, bank_lds, enc, out,
                           (long)out_stride);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_deliver");
    }
    if (state_pool) {
        ProfScope ps(st, "deliver_carry", 0.0, 8.0 * B * (klen - 1));
        hipLaunchKernelGGL(deliver_carry_kernel, dim3((unsigned)B), dim3(256), (size_t)(klen - 1) * sizeof(float), st, audio,
                           (long)row_stride, table, klen - 1, static_cast<char*>(state_pool), slot_stride, (long)n_slots);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_deliver");
    }
    return 0;
}

}  // extern "C"
