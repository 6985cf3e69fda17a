// Pitch (DESIGN '8o. Pitch'), gfx950: normalised cross-correlation scores of the 24 kHz waveform and the best path through them, an F0
// track of one lag (or "unvoiced") per frame.  The contract is written out in include/smalltts_hip.h (smtts_pitch); this file is the
// two kernels and the entries.  Plain C++, no atomics, nothing scheduling-dependent.
//
// pitch_score_kernel: one workgroup of PS_THREADS threads per row and tile of PS_T frames.  The tile's samples x[s0, s0 + (T - 1) hop +
// win + lmax) are staged in LDS once, +0.0 from n on (nothing behind n is loaded, and no later stage needs a bounds check).  The
// (frame, lag) pairs of the tile are dealt out to the threads in order, lags fastest: consecutive lanes read candidates at stride 1
// (consecutive banks), and the frame's template comes as ds_read_b128 from one address in all lanes of a frame (a broadcast; a wave
// that straddles two frames reads two addresses).  Twelve independent fmaf chains per lane: four each for r, e and e0.
//
// pitch_path_kernel: one workgroup per row walks the row's frames in order.  D lies double-buffered in LDS next to lg; a thread owns
// one state j and a share (one of `parts`) of its predecessors, which it scans as float4 broadcasts; the shares are combined through
// LDS in ascending order with a strict compare, so that the smallest j' wins a tie whatever the split.  The minimum of a set of floats
// does not depend on the order it is taken in, so this is the header's direct form bit for bit.  Back pointers go to the workspace as
// uint16 (F, L + 1); the trace reads them back through LDS in chunks of PP_CHUNK_BYTES (thread 0 walks a chunk, then every thread
// writes one frame's lag and peak), so that the chain of dependent loads runs on LDS, not on global memory.
#include "../../include/smalltts_hip.h"

#include <cmath>
#include <cstdint>

#include "capi_handle.hpp"
#include "prof.hpp"

// The local cost and the transition are separately rounded fp32 operations (the header).  hipcc contracts a * b + c into an fma by
// default; the pragma keeps the plain operators of this file apart (retime.hip has the long version).  What wants an fma asks for fmaf
// by name, as the dot products do.
#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = 256, PS_T = 8;
constexpr int PP_MAX_STATES = 1024;                 // L + 1 <= 1024
constexpr int PP_CHUNK_BYTES = 32768;               // back pointers the trace holds in LDS at a time
constexpr int PP_CHUNK_FRAMES = 1024;               // ... and at most so many frames of them
constexpr int PT_MAX_HOP = 1024, PT_MAX_WIN = 2048, PT_MAX_LAG = 2048;

__device__ __forceinline__ long pt_clamp(long v, long lo, long hi) { return v < lo ? lo : v > hi ? hi : v; }
__host__ __device__ inline size_t pt_up256(size_t v) { return (v + 255) & ~(size_t)255; }

__global__ __launch_bounds__(PS_THREADS) void pitch_score_kernel(const float* __restrict__ audio, long row_stride,
                                                                 const int64_t* __restrict__ len, int hop, int win, int lmin, int L,
                                                                 float bias, float* __restrict__ S, long Fmax) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long n = pt_clamp((long)len[b], 0, row_stride);
    const long F = (n + hop - 1) / hop;
    const long f0 = (long)blockIdx.x * PS_T;
    if (f0 >= F) return;                                       // the same for every thread of the workgroup
    const int T = F - f0 < PS_T ? (int)(F - f0) : PS_T;
    const long s0 = f0 * hop;
    const float* const x = audio + (long)b * row_stride;
    const int cnt = (T - 1) * hop + win + lmin + L - 1;        // <= 7 * 1024 + 2048 + 2048 floats, the launch's dynamic LDS
    for (int i = tid; i < cnt; i += PS_THREADS) xs[i] = s0 + i < n ? x[s0 + i] : 0.0f;
    __syncthreads();
    float* const out = S + ((long)b * Fmax + f0) * L;
    for (int item = tid; item < T * L; item += PS_THREADS) {
        const int t = item / L, c = item - t * L;
        const float* const tm = xs + t * hop;                  // hop % 4 == 0: 16-byte aligned
        const float* const cd = tm + lmin + c;
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f, e0 = 0.0f, e1 = 0.0f, e2 = 0.0f, e3 = 0.0f;
        float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f, z3 = 0.0f;     // the order of the sums is free
        for (int i = 0; i < win; i += 4) {
            const float4 v = *reinterpret_cast<const float4*>(tm + i);
            const float c0 = cd[i], c1 = cd[i + 1], c2 = cd[i + 2], c3 = cd[i + 3];
            r0 = fmaf(v.x, c0, r0);
            r1 = fmaf(v.y, c1, r1);
            r2 = fmaf(v.z, c2, r2);
            r3 = fmaf(v.w, c3, r3);
            e0 = fmaf(c0, c0, e0);
            e1 = fmaf(c1, c1, e1);
            e2 = fmaf(c2, c2, e2);
            e3 = fmaf(c3, c3, e3);
            z0 = fmaf(v.x, v.x, z0);
            z1 = fmaf(v.y, v.y, z1);
            z2 = fmaf(v.z, v.z, z2);
            z3 = fmaf(v.w, v.w, z3);
        }
        const float r = (r0 + r1) + (r2 + r3), e = (e0 + e1) + (e2 + e3), z = (z0 + z1) + (z2 + z3);
        out[item] = r / sqrtf(z * e + bias);                   // item = t * L + c: the tile's frames lie one behind the other
    }
}

__global__ __launch_bounds__(PP_MAX_STATES) void pitch_path_kernel(const float* __restrict__ S, const int64_t* __restrict__ len,
                                                                   long row_stride, const float* __restrict__ tab, int hop, int lmin, int L,
                                                                   int nsp, int parts, float c_unv, float w_jump, float w_switch,
                                                                   unsigned short* __restrict__ bp, int* __restrict__ lag,
                                                                   float* __restrict__ peak, long Fmax) {
    __shared__ __attribute__((aligned(16))) float Db[2][PP_MAX_STATES + 4];
    __shared__ __attribute__((aligned(16))) float lgs[PP_MAX_STATES + 4];      // lgs[j] = lg of state j; lgs[0] is not used
    __shared__ float pbest[PP_MAX_STATES];
    __shared__ unsigned short parg[PP_MAX_STATES];
    __shared__ unsigned short chunk[PP_CHUNK_BYTES / 2];
    __shared__ unsigned short cst[PP_CHUNK_FRAMES];                           // the states of a chunk's frames
    __shared__ int sh_state;
    const int b = blockIdx.x, tid = threadIdx.x;
    const long n = pt_clamp((long)len[b], 0, row_stride);
    const long F = (n + hop - 1) / hop;
    if (F == 0) return;                                        // the same for every thread of the workgroup
    const int NS = L + 1;
    const int NS4 = (NS + 3) & ~3;
    const int j = tid % nsp, part = tid / nsp;                 // this thread's state and its share of the predecessors
    const bool owner = part == 0 && j < NS;
    const bool isz = j == 0;
    // a share: predecessors [a, e), both multiples of 4; the shares cover [0, NS4)
    const int per = ((NS4 / 4 + parts - 1) / parts) * 4;
    const int a = part * per, e = a + per < NS4 ? a + per : NS4;
    const float* const Sr = S + (long)b * Fmax * L;
    unsigned short* const bpr = bp + (long)b * Fmax * NS;
    // the table is clamped as it is loaded, never trusted: lg into [0, 16], tilt into [0, 2], a NaN reads as 0
    float lgj = 0.0f, tiltj = 0.0f;
    if (j >= 1 && j < NS) {
        lgj = fminf(fmaxf(tab[j - 1], 0.0f), 16.0f);
        tiltj = fminf(fmaxf(tab[L + j - 1], 0.0f), 2.0f);
    }
    for (int i = tid; i < NS4; i += blockDim.x) {
        lgs[i] = (i >= 1 && i < NS) ? fminf(fmaxf(tab[i - 1], 0.0f), 16.0f) : 0.0f;
        Db[0][i] = INFINITY;                                   // the padding behind NS stays +inf in both buffers: it never wins
        Db[1][i] = INFINITY;
    }
    __syncthreads();
    auto loc = [&](float s) -> float {                         // the local cost of this thread's state given its score
        if (isz) return c_unv;
        const float p = s * tiltj;
        const float v = 1.0f - p;
        return v == v ? v : INFINITY;                          // a NaN cost counts as +inf
    };
    float s_next = (owner && !isz) ? Sr[j - 1] : 0.0f;
    if (owner) Db[0][j] = loc(s_next);
    if (owner && !isz && F > 1) s_next = Sr[L + j - 1];
    __syncthreads();
    for (long f = 1; f < F; ++f) {
        const float* const Dp = Db[(f - 1) & 1];
        float* const Dn = Db[f & 1];
        const float s_cur = s_next;
        if (owner && !isz && f + 1 < F) s_next = Sr[(f + 1) * L + j - 1];   // on its way while the predecessors are scanned
        float best = INFINITY;
        int arg = a;
        if (j < NS) {
            for (int q = a; q < e; q += 4) {
                const float4 d = *reinterpret_cast<const float4*>(Dp + q);
                const float4 g = *reinterpret_cast<const float4*>(lgs + q);
                // predecessor 0 (q == 0, .x): 0 -> 0 costs 0, 0 -> j costs w_switch; a voiced predecessor: w_switch into state 0
                float t0 = isz ? w_switch : w_jump * fabsf(lgj - g.x);
                if (q == 0) t0 = isz ? 0.0f : w_switch;
                const float t1 = isz ? w_switch : w_jump * fabsf(lgj - g.y);
                const float t2 = isz ? w_switch : w_jump * fabsf(lgj - g.z);
                const float t3 = isz ? w_switch : w_jump * fabsf(lgj - g.w);
                const float c0 = d.x + t0, c1 = d.y + t1, c2 = d.z + t2, c3 = d.w + t3;
                if (c0 < best) { best = c0; arg = q; }         // strict: the smallest j' keeps a tie
                if (c1 < best) { best = c1; arg = q + 1; }
                if (c2 < best) { best = c2; arg = q + 2; }
                if (c3 < best) { best = c3; arg = q + 3; }
            }
        }
        if (parts > 1) {
            pbest[tid] = best;
            parg[tid] = (unsigned short)arg;
            __syncthreads();
            if (owner) {
                for (int p = 1; p < parts; ++p) {              // ascending shares, strict compare: the smallest j' again
                    const float o = pbest[p * nsp + j];
                    if (o < best) { best = o; arg = parg[p * nsp + j]; }
                }
            }
        }
        if (owner) {
            Dn[j] = loc(s_cur) + best;
            bpr[f * NS + j] = (unsigned short)arg;
        }
        __syncthreads();                                       // Dn is complete; pbest / parg and Dp may be written again
    }
    // the end: the smallest j among the minima of D[F - 1]
    if (tid == 0) {
        const float* const Dl = Db[(F - 1) & 1];
        float best = Dl[0];
        int arg = 0;
        for (int q = 1; q < NS; ++q)
            if (Dl[q] < best) { best = Dl[q]; arg = q; }
        sh_state = arg;
    }
    __syncthreads();                                           // also: every back pointer of this workgroup is written (same workgroup reads)
    const int CH = PP_CHUNK_BYTES / 2 / NS < PP_CHUNK_FRAMES ? PP_CHUNK_BYTES / 2 / NS : PP_CHUNK_FRAMES;   // frames of a chunk: 16 .. 1024
    int* const lr = lag + (long)b * Fmax;
    float* const pr = peak + (long)b * Fmax * 3;
    for (long hi = F - 1; hi >= 0; hi -= CH) {                 // frames (hi - cn, hi], from the back
        const int cn = hi + 1 < CH ? (int)(hi + 1) : CH;
        const long lo = hi - cn + 1;
        // back pointers of frames lo + 1 .. hi (frame 0 has none); rows lie one behind the other
        const long first = lo > 0 ? lo : 1;
        const int rows = (int)(hi - first + 1);
        const unsigned short* const src = bpr + first * NS;
        for (int i = tid; i < rows * NS; i += blockDim.x) chunk[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            int q = sh_state;                                  // the state of frame hi
            for (long f = hi; f >= lo; --f) {
                cst[f - lo] = (unsigned short)q;
                if (f >= first) {                              // step to frame f - 1 (clamped: whatever the workspace held)
                    int m = chunk[(f - first) * NS + q];
                    q = m > L ? L : m;
                }
            }
            sh_state = q;                                      // the state of frame lo - 1 (not used behind frame 0)
        }
        __syncthreads();
        for (int i = tid; i < cn; i += blockDim.x) {
            const long f = lo + i;
            const int q = cst[i];
            float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
            if (q > 0) {
                const float* const sf = Sr + f * L;
                const int c = q - 1;
                p1 = sf[c];
                p0 = c > 0 ? sf[c - 1] : p1;
                p2 = c + 1 < L ? sf[c + 1] : p1;
            }
            lr[f] = q > 0 ? lmin + q - 1 : 0;
            pr[3 * f] = p0;
            pr[3 * f + 1] = p1;
            pr[3 * f + 2] = p2;
        }
        __syncthreads();                                       // chunk / cst are free again
    }
}

// why the shape is refused, or nullptr
const char* pt_shape(int B, int64_t row_stride, int hop, int lmin, int lmax) {
    if (B < 1 || B > 1024) return "B must be in [1, 1024]";
    if (row_stride < 1 || row_stride > (int64_t)1 << 24) return "row_stride must be in [1, 2^24]";
    if (hop < 16 || hop > PT_MAX_HOP || hop % 4) return "hop must be a multiple of 4 in [16, 1024]";
    if (lmin < 2 || lmax <= lmin || lmax > PT_MAX_LAG || lmax - lmin + 1 > PP_MAX_STATES - 1)
        return "lags must satisfy 2 <= lmin < lmax <= 2048 and lmax - lmin + 1 <= 1023";
    return nullptr;
}

struct PtPlan {
    size_t s_bytes, bp_bytes;
    long Fmax;
};
PtPlan pt_plan(int B, int64_t row_stride, int hop, int lmin, int lmax) {
    const long L = lmax - lmin + 1, Fmax = (long)((row_stride + hop - 1) / hop);
    return {pt_up256((size_t)B * Fmax * L * sizeof(float)), pt_up256((size_t)B * Fmax * (L + 1) * sizeof(unsigned short)), Fmax};
}

}  // namespace

extern "C" {

size_t smtts_pitch_workspace_bytes(smtts_handle h, int B, int64_t row_stride, int hop, int lmin, int lmax) { NULLCHK0;
    if (const char* why = pt_shape(B, row_stride, hop, lmin, lmax)) {
        E.fail(std::string("smtts_pitch_workspace_bytes: ") + why);
        return 0;
    }
    const PtPlan p = pt_plan(B, row_stride, hop, lmin, lmax);
    return p.s_bytes + p.bp_bytes;
}

int smtts_pitch(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, const float* tab, int hop,
                int win, int lmin, int lmax, float bias, float c_unv, float w_jump, float w_switch, int32_t* lag, float* peak, float* nccf,
                void* ws, size_t ws_bytes) { NULLCHK;
    if (!audio || !len || !tab || !lag || !peak || !ws) return E.fail("smtts_pitch: a required pointer is NULL");
    if (const char* why = pt_shape(B, row_stride, hop, lmin, lmax)) return E.fail(std::string("smtts_pitch: ") + why);
    if (win < 32 || win > PT_MAX_WIN || win % 4) return E.fail("smtts_pitch: win must be a multiple of 4 in [32, 2048]");
    if (!(bias > 0.0f) || !std::isfinite(bias)) return E.fail("smtts_pitch: bias must be positive and finite");
    if (!(c_unv >= 0.0f) || !std::isfinite(c_unv) || !(w_jump >= 0.0f) || !std::isfinite(w_jump) || !(w_switch >= 0.0f) ||
        !std::isfinite(w_switch))
        return E.fail("smtts_pitch: c_unv, w_jump and w_switch must be non-negative and finite");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return E.fail("smtts_pitch: the workspace must be 256-byte aligned");
    const PtPlan p = pt_plan(B, row_stride, hop, lmin, lmax);
    if (ws_bytes < p.s_bytes + p.bp_bytes) return E.fail("smtts_pitch: workspace smaller than smtts_pitch_workspace_bytes");
    const int L = lmax - lmin + 1;
    float* const S = nccf ? nccf : static_cast<float*>(ws);
    unsigned short* const bp = reinterpret_cast<unsigned short*>(static_cast<char*>(ws) + p.s_bytes);
    hipStream_t st = ST(stream);
    {
        const long tiles = (p.Fmax + PS_T - 1) / PS_T;         // <= 2^24 / 16 / 8
        const size_t lds = ((size_t)(PS_T - 1) * hop + win + lmax) * sizeof(float);   // <= 45056 bytes
        ProfScope ps(st, "pitch_score", 6.0 * B * (double)p.Fmax * L * win, 4.0 * B * ((double)row_stride + (double)p.Fmax * L));
        hipLaunchKernelGGL(pitch_score_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(PS_THREADS), lds, st, audio, (long)row_stride, len,
                           hop, win, lmin, L, bias, S, p.Fmax);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_pitch");
    }
    {
        const int nsp = (L + 1 + 63) / 64 * 64;                // threads of one share: a thread per state, whole waves
        int parts = PP_MAX_STATES / nsp;
        parts = parts > 4 ? 4 : parts;
        ProfScope ps(st, "pitch_path", 4.0 * B * (double)p.Fmax * (L + 1) * (L + 1), B * (double)p.Fmax * (4.0 * L + 4.0 * (L + 1)));
        hipLaunchKernelGGL(pitch_path_kernel, dim3((unsigned)B), dim3(nsp * parts), 0, st, S, len, (long)row_stride, tab, hop, lmin, L, nsp,
                           parts, c_unv, w_jump, w_switch, bp, lag, peak, p.Fmax);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return E.fail_hip(e, "smtts_pitch");
    }
    return 0;
}

}  // extern "C"
