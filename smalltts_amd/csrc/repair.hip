// Repair: re-speak only the badly aligned words of a take, on the device (DESIGN '8e. Repair'), gfx950.
//
// repair_plan: behind align_path (and take_select), one workgroup of 256 threads per row.  From the tapped text mass (B, N, P) and the
// path's spans (B, P, 2) it decides which tokens of the row's window (frames [0, n), tokens [p0, p1), clamped as take_scores clamps
// them) are bad: an empty span, a span longer than max_span, or a span no frame of which attends to the token (no mass[f][p] >=
// tau_tok, one fp32 comparison; a NaN never attends).  A bad token with a span frees its frames plus `margin` on either side; every
// other frame below n, and every frame the caller's keep mask names, is pinned.  -> pin u8 (B, N), the mask smtts_sample_pinned
// takes, every byte of the row written, and counts (B, 2) = (bad tokens, freed frames).  Loads: thread = token walking down its span
// (adjacent lanes read adjacent floats of a mass row), the freed ranges are plain stores of 1 into an LDS flag per frame (overlaps
// store the same value), then thread = frame writes the mask.
//
// repair_keep: grid (chunks, G).  Every workgroup re-derives replace[g] = counts[g][1] > 0 && key(total_new[g]) < key(total_cur[g])
// (key = NaN ? +inf : total; strict <: ties keep the current row) from inputs nobody writes, and where it holds copies its chunk of
// row g of x_new (N, 64), spans_new (P, 2) and mass_new (N, P) over the current row in place, in 16-byte lanes where the row's byte
// count and both bases allow and in 4-byte elements otherwise.  total_out / feat_out are those of the row that stays, kept = replace.
// Plain VALU + LDS, no atomics: two runs return the same bits whatever else the chip is doing.
#include <algorithm>

#include "kernels.hpp"
#include "prof.hpp"
#include "row_copy.hpp"

namespace {

constexpr int RP_MAXN = 225, RP_MAXP = 198, RP_NT = 256;   // align_path's range: one thread per token, then one per frame

__global__ __launch_bounds__(RP_NT) void repair_plan_kernel(const float* __restrict__ mass, const int* __restrict__ spans,
                                                            const int* __restrict__ n_len, const int* __restrict__ p0a,
                                                            const int* __restrict__ p1a, const uint8_t* __restrict__ keep, int N, int P,
                                                            float tau_tok, int max_span, int margin, uint8_t* __restrict__ pin,
                                                            int* __restrict__ counts) {
    __shared__ int freed[RP_NT];          // per frame: some bad token frees it
    __shared__ int part[2][RP_NT / 64];   // per wave: bad tokens, freed frames
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int nb = n_len[b], p0 = p0a[b], p1 = p1a[b];
    nb = nb < 0 ? 0 : nb > N ? N : nb;
    p0 = p0 < 0 ? 0 : p0 > P ? P : p0;
    p1 = p1 < 0 ? 0 : p1 > P ? P : p1;
    const int Pw = p1 - p0;
    uint8_t* const prow = pin + (long)b * N;
    if (nb <= 0 || Pw <= 0) {   // (uniform)
        if (t < N) prow[t] = 0;
        if (t < 2) counts[(long)b * 2 + t] = 0;
        return;
    }
    freed[t] = 0;
    __syncthreads();
    const float* const mrow = mass + (long)b * N * P;   // every index below: frame in [0, nb) <= N, token in [p0, p1) <= P
    // thread = token: is it bad, and which frames does it free
    int bad = 0;
    if (t < Pw) {
        const int p = p0 + t;
        int first = spans[((long)b * P + p) * 2], last = spans[((long)b * P + p) * 2 + 1];
        bad = 1;
        if (first >= 0 && last >= first) {
            first = first > nb - 1 ? nb - 1 : first;   // (first >= 0 already)
            last = last > nb - 1 ? nb - 1 : last;
            if (last - first + 1 <= max_span) {
                for (int f = first; f <= last; ++f)
                    if (mrow[(long)f * P + p] >= tau_tok) bad = 0;
            }
            if (bad) {
                const int lo = first - margin < 0 ? 0 : first - margin, hi = last + margin > nb - 1 ? nb - 1 : last + margin;
                for (int f = lo; f <= hi; ++f) freed[f] = 1;
            }
        }
    }
    __syncthreads();
    // thread = frame
    int open = 0;
    if (t < N) {
        int v = 0;
        if (t < nb) {
            v = !freed[t] || (keep && keep[(long)b * N + t] != 0);
            open = !v;
        }
        prow[t] = (uint8_t)v;
    }
    const int bad_w = wave_sum(bad), open_w = wave_sum(open);
    if (lane == 0) { part[0][w] = bad_w; part[1][w] = open_w; }
    __syncthreads();
    if (t < 2) {
        int s = 0;
        for (int i = 0; i < RP_NT / 64; ++i) s += part[t][i];
        counts[(long)b * 2 + t] = s;
    }
}

__global__ __launch_bounds__(RP_NT) void repair_keep_kernel(const uint32_t* __restrict__ total_cur, const uint32_t* __restrict__ total_new,
                                                            const int* __restrict__ counts, const int* __restrict__ feat_cur,
                                                            const int* __restrict__ feat_new, RowCopy x, RowCopy sp, RowCopy ms,
                                                            uint32_t* __restrict__ total_out, int* __restrict__ feat_out,
                                                            int* __restrict__ kept) {
    const int g = blockIdx.y, t = threadIdx.x;
    float a = __uint_as_float(total_cur[g]), c = __uint_as_float(total_new[g]);
    a = a != a ? INFINITY : a;
    c = c != c ? INFINITY : c;
    const bool replace = counts[(long)g * 2 + 1] > 0 && c < a;   // (uniform: every workgroup of the row decides alike)
    if (replace) {
        row_copy(x, g, g, RP_NT);
        row_copy(sp, g, g, RP_NT);
        row_copy(ms, g, g, RP_NT);
    }
    if (blockIdx.x == 0) {
        if (t < 4) feat_out[(long)g * 4 + t] = (replace ? feat_new : feat_cur)[(long)g * 4 + t];
        if (t == 0) {
            total_out[g] = (replace ? total_new : total_cur)[g];   // (the stored bits, a NaN's payload included)
            kept[g] = replace ? 1 : 0;
        }
    }
}

}  // namespace

hipError_t launch_repair_plan(const float* mass, const int* spans, const int* n_len, const int* p0, const int* p1, const uint8_t* keep,
                              int B, int N, int P, float tau_tok, int max_span, int margin, uint8_t* pin, int* counts, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (N < 1 || P < 1 || N > RP_MAXN || P > RP_MAXP || max_span < 1 || margin < 0) return hipErrorInvalidValue;
    ProfScope ps(st, "repair_plan", 1.0 * B * N * P, 4.0 * B * N * P);
    hipLaunchKernelGGL(repair_plan_kernel, dim3(B), dim3(RP_NT), 0, st, mass, spans, n_len, p0, p1, keep, N, P, tau_tok, max_span, margin,
                       pin, counts);
    return hipGetLastError();
}

hipError_t launch_repair_keep(int G, int N, int P, const float* total_cur, const float* total_new, const int* counts, const int* feat_cur,
                              const int* feat_new, float* x_cur, const float* x_new, int* spans_cur, const int* spans_new, float* mass_cur,
                              const float* mass_new, float* total_out, int* feat_out, int* kept, hipStream_t st) {
    if (G <= 0) return hipSuccess;
    if (N < 1 || P < 1 || N > RP_MAXN || P > RP_MAXP || G > 65535) return hipErrorInvalidValue;
    if ((spans_cur != nullptr) != (spans_new != nullptr) || (mass_cur != nullptr) != (mass_new != nullptr)) return hipErrorInvalidValue;
    const RowCopy cx = make_row_copy(x_new, x_cur, (long)N * 64), cs = make_row_copy(spans_new, spans_cur, (long)P * 2),
                  cm = make_row_copy(mass_new, mass_cur, (long)N * P);
    // lanes of the widest copy, four to a thread
    long units = cx.vec ? cx.n4 / 4 : cx.n4;
    if (cm.src) units = std::max(units, cm.vec ? cm.n4 / 4 : cm.n4);
    const int chunks = (int)std::min<long>(64, std::max<long>(1, (units + 4 * RP_NT - 1) / (4 * RP_NT)));
    const double bytes = 4.0 * G * (cx.n4 + (cs.src ? cs.n4 : 0) + (cm.src ? cm.n4 : 0));
    ProfScope ps(st, "repair_keep", 0.0, 2.0 * bytes);
    hipLaunchKernelGGL(repair_keep_kernel, dim3(chunks, G), dim3(RP_NT), 0, st, reinterpret_cast<const uint32_t*>(total_cur),
                       reinterpret_cast<const uint32_t*>(total_new), counts, feat_cur, feat_new, cx, cs, cm,
                       reinterpret_cast<uint32_t*>(total_out), feat_out, kept);
    return hipGetLastError();
}
