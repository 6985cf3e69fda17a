// Engine internals shared by the engine*.hip units (engine.hpp stays the class declaration): the error macro, the workspace bump
// allocator, the small helpers that build GEMM calls, and the workspace structs that more than one unit plans with.  Not installed,
// not included by anything outside the engine units.
#pragma once
#include "engine.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

// LN-fold row shift (gemm.hpp LnFoldIn::cshift).  -DLN_FOLD_SHIFT=0 builds the unshifted fold of round 6 (A/B of the precision
// tests only: tests/test_ln_fold_gpu.py measures both against fp64)
#ifndef LN_FOLD_SHIFT
#define LN_FOLD_SHIFT 1
#endif
#define HIPC(x)                                          \
    do {                                                 \
        hipError_t e__ = (x);                            \
        if (e__ != hipSuccess) return fail_hip(e__, #x); \
    } while (0)

struct Bump {  // bump allocator over a caller-owned workspace (also used, with p == null, to size it)
    char* p;
    size_t off = 0;
    explicit Bump(void* base) : p(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* r = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + off);   // (integer arithmetic: the sizing run's base is null)
        off += n * sizeof(T);
        return r;
    }
};
// Bump aligns its offsets relative to the base and the operand-format tag rides in the low bits of a carve-out's address
// (common.hpp sm_lo_for): both hold only on a 256-byte aligned workspace.  Checked by every operator next to its size check.
inline bool ws_misaligned(const void* ws) { return (reinterpret_cast<uintptr_t>(ws) & 255) != 0; }
inline std::string sidx(const std::string& a, int i, const std::string& b) { return a + std::to_string(i) + b; }

std::vector<int> swiglu_perm(int F);   // engine_finalize.hip

// ---------------------------------------------------------------------------------------------
// small helpers to build GEMM calls
// ---------------------------------------------------------------------------------------------
static inline GemmOperands ops(const float* A, RowMap amap, const PW& w, int M, int row0 = 0, int nrows = -1) {
    GemmOperands g;
    g.A = A;
    g.amap = amap;
    g.Whi = w.hi + (long)row0 * w.K;
    g.Wlo = w.lo + (long)row0 * w.K;
    g.ldw = w.K;
    g.M = M;
    g.N = nrows < 0 ? w.N : nrows;
    g.K = w.K;
    g.a_z = 0;
    g.w_z = 0;
    g.w_zmod = 0;
    return g;
}
struct SplitBuf {  // activation buffer feeding gemm3 as its A operand: a split bf16 pair (x ~= hi + lo), or — for a consumer
    bf16_t* hi;     // of precision PREC_F16 / PREC_BF16 — one 16-bit array in `hi` (`lo` allocated but unused)
    bf16_t* lo;
    // the (hi, lo) pair a PRODUCER is handed so that it writes the format a consumer of precision `prec` reads (common.hpp)
    // (`sat`: the consumer site's saturation counter, counted into by fp16 producers — common.hpp sat_note)
    SplitBuf as(int prec, unsigned* sat = nullptr) const { return SplitBuf{hi, sm_lo_for(prec, lo, sat)}; }
};
static inline Gemm3Operands ops3(SplitBuf a, RowMap amap, const PW& w, int M, int prec, int row0 = 0, int nrows = -1) {
    Gemm3Operands g;
    g.Ahi = a.hi;
    g.Alo = prec == PREC_BF16X3 ? a.lo : nullptr;
    g.amap = amap;
    g.Whi = (prec == PREC_F16 ? w.h16 : w.hi) + (long)row0 * w.K;
    g.Wlo = prec == PREC_BF16X3 ? w.lo + (long)row0 * w.K : nullptr;
    g.ldw = w.K;
    g.M = M;
    g.N = nrows < 0 ? w.N : nrows;
    g.K = w.K;
    g.a_z = 0;
    g.w_z = 0;
    g.w_zmod = 0;
    g.ksplit_tiles = 0;
    return g;
}
static inline EpiStore<ACT_NONE> store_to(float* out, RowMap omap, const float* bias, float scale = 1.f,
                                          const uint8_t* rowmask = nullptr) {
    return EpiStore<ACT_NONE>{out, omap, 0, bias, 0, scale, rowmask, nullptr, nullptr};
}
static inline EpiStore<ACT_NONE> store_split_to(SplitBuf o, RowMap omap, const float* bias, float scale = 1.f,
                                                const uint8_t* rowmask = nullptr) {
    return EpiStore<ACT_NONE>{nullptr, omap, 0, bias, 0, scale, rowmask, o.hi, o.lo};
}
template <class T>
static inline SplitBuf take_split(T& bump, size_t elems) {
    SplitBuf s;
    s.hi = bump.template take<bf16_t>(elems);
    s.lo = bump.template take<bf16_t>(elems);
    return s;
}

// Split-K residual GEMM for the small-M DiT projections (N = 960 gives only 150 tiles): the K range is cut into
// `splits` slices (grid.z), each writes an fp32 partial, and one fused kernel reduces them in a fixed order and
// applies bias / tanh-gate / row mask / residual add -> deterministic, unlike atomics.
struct NextLN {  // optional: the AdaLN that follows the residual, fused into the split-K reduction kernel
    const float* shift = nullptr;
    const float* scale = nullptr;
    bf16_t* yhi = nullptr;
    bf16_t* ylo = nullptr;
    bool rms = false;   // true: RMSNorm with weight `shift` (encoders) instead of LayerNorm * (1 + scale) + shift
    float eps = 1e-6f;
};
static hipError_t gemm3_resid_splitk(const Gemm3Operands& g0, const EpiResid<0>& r, float* partial, int splits, int split,
                                     hipStream_t st, const LaunchTuning& tu, const NextLN& ln = NextLN(), int cfg = G3_64x64) {
    Gemm3Operands g = g0;
    const int nk = g.K / 64;
    g.ksplit_tiles = (nk + splits - 1) / splits;
    const int used = (nk + g.ksplit_tiles - 1) / g.ksplit_tiles;
    EpiStore<ACT_NONE> e{partial, rowmap_plain(g.N), (long)g.M * g.N, nullptr, 0, 1.f, nullptr, nullptr, nullptr};
    hipError_t err = gemm3_store(g, ACT_NONE, e, used, split, st, tu, cfg);
    if (err != hipSuccess) return err;
    if (ln.shift)
        return launch_splitk_resid_ln(partial, used, r.x, r.bias, r.gate, r.gld, r.grow0, r.grstride, r.rows_per_batch,
                                      r.rowmask, g.M, g.N, ln.eps, ln.shift, ln.scale, ln.yhi, ln.ylo, st, ln.rms);
    return launch_splitk_resid(partial, used, r.x, r.bias, r.gate, r.gld, r.grow0, r.grstride, r.rows_per_batch, r.rowmask,
                               g.M, g.N, st, &r.xmap);
}

// K slices that spread a weight-bound product (few rows, long K) over the chip.  The count depends on (K, row class) only, never
// on M itself, so that results stay bit-identical across batch sizes inside a class (tests/test_fullsize_gpu.py: a batch of 2
// shares its prefix with the batch of 1).  Slices of >= 16 k-tiles (>= 32 in the 513..2048-row class).  1 = leave the product alone.
static int small_m_splits(int M, int K, int max_few, int max_some) {
    const int nk = K / 64;
    int sp = 1;
    if (M <= 512) sp = nk / 16 < max_few ? nk / 16 : max_few;
    else if (M <= 2048) sp = nk / 32 < max_some ? nk / 32 : max_some;
    return sp < 2 ? 1 : sp;
}
// out = A x W^T + bias as K slices into fp32 partials + one fixed-order reduce pass (no residual: the reduce overwrites)
static hipError_t gemm3_store_splitk(const Gemm3Operands& g0, float* partial, int splits, int split, const float* bias, float* out,
                                     const RowMap& omap, hipStream_t st, const LaunchTuning& tu) {
    Gemm3Operands g = g0;
    const int nk = g.K / 64;
    g.ksplit_tiles = (nk + splits - 1) / splits;
    const int used = (nk + g.ksplit_tiles - 1) / g.ksplit_tiles;
    EpiStore<ACT_NONE> e{partial, rowmap_plain(g.N), (long)g.M * g.N, nullptr, 0, 1.f, nullptr, nullptr, nullptr};
    hipError_t err = gemm3_store(g, ACT_NONE, e, used, split, st, tu, G3_64x64);
    if (err != hipSuccess) return err;
    return launch_splitk_resid(partial, used, out, bias, nullptr, 0, 0, 0, 1, nullptr, g.M, g.N, st, &omap, true);
}

// ---------------------------------------------------------------------------------------------
// workspaces: plan() on a Bump over a null base sizes, the same plan() over the caller's workspace carves
// ---------------------------------------------------------------------------------------------
struct Engine::EncWs {
    float *x, *qkvg, *seq, *part, *lnpart;
    SplitBuf y, o, ffh, seqs;
    SplitBuf qi, ki, vti, gi;   // attention operand images (attention_img.hip): [B][H][S][dhp] x 2, [B][H][dhp][pad8(S)], [M][D]
    size_t vt_elems;
    void plan(Bump& b, int B, int S) {
        const int Mx = B * S > 0 ? B * S : 1;
        x = b.take<float>((size_t)Mx * 512);
        part = b.take<float>((size_t)kSplitK * Mx * 512);
        lnpart = b.take<float>((size_t)Mx * (512 / 32) * 2);
        qkvg = b.take<float>((size_t)Mx * 2048);
        seq = b.take<float>((size_t)Mx * kHidden);
        y = take_split(b, (size_t)Mx * 512);
        o = take_split(b, (size_t)Mx * 512);
        ffh = take_split(b, (size_t)Mx * 1536);
        seqs = take_split(b, (size_t)Mx * kHidden);
        // H * dhp = 512 for both encoders (8 x 64, 4 x 128); V^T rows are padded to 8 keys per utterance: B x 512 x pad8(S)
        // (round 3 took 8 Mx x 512 here, "at most Mx + 7 B <= 8 Mx": 16 KB per row, GBs at large B x P — ADVICE r3)
        qi = take_split(b, (size_t)Mx * 512);
        ki = take_split(b, (size_t)Mx * 512);
        vt_elems = (size_t)(B > 0 ? B : 1) * 512 * (size_t)pad8(S > 0 ? S : 1);
        vti = take_split(b, vt_elems);
        gi = take_split(b, (size_t)Mx * 512);
    }
};

struct Engine::ModWs {
    float *sinb, *t1, *temb, *e1, *semb, *mod, *ftab = nullptr;
    void plan(Bump& b, int rows, bool fold = false) {
        if (fold) ftab = b.take<float>((size_t)rows * 2 * kFoldNF);
        sinb = b.take<float>((size_t)rows * 256);
        t1 = b.take<float>((size_t)rows * kHidden);
        temb = b.take<float>((size_t)rows * kHidden);
        e1 = b.take<float>((size_t)rows * 2 * kHidden);
        semb = b.take<float>((size_t)rows * kHidden);
        mod = b.take<float>((size_t)rows * kModLd);
    }
};

struct Engine::CoreWs {
    float *h, *x, *qkvg, *part, *lnpart, *lnc;   // lnc [M]: the LN-fold producers' row shift (gemm.hpp LnFoldIn::cshift)
    float *rope_c, *rope_s;  // cos / sin of a caller-supplied angle table: per call (several calls may be in flight on different streams)
    SplitBuf gm1, gm2, y, o, ffh;
    SplitBuf qi, ki, vti, gi;   // attention operand images of the self part: [B][8][N][128] x 2, [B][8][128][pad8(N)], [M][960]
    size_t gm_elems, vt_elems;
    void plan(Bump& b, int B, int N) {
        const size_t M = (size_t)B * N;
        qi = take_split(b, M * kHeads * 128);
        ki = take_split(b, M * kHeads * 128);
        vt_elems = (size_t)B * kHeads * 128 * pad8(N);
        vti = take_split(b, vt_elems);
        gi = take_split(b, M * kHidden);
        gm_elems = (size_t)B * kConvG * (N + 2 * kConvPad) * kConvGs;
        h = b.take<float>(M * kHidden);
        x = b.take<float>(M * kHidden);
        qkvg = b.take<float>(M * 4 * kHidden);
        part = b.take<float>(M * kHidden * kSplitK);
        lnpart = b.take<float>(M * kLnGroups * 2);
        lnc = b.take<float>(M);
        rope_c = b.take<float>((size_t)N * 64);
        rope_s = b.take<float>((size_t)N * 64);
        gm1 = take_split(b, gm_elems);
        gm2 = take_split(b, gm_elems);
        y = take_split(b, M * kHidden);
        o = take_split(b, M * kHidden);
        ffh = take_split(b, M * kFFp);
    }
};

// (a part of DitWs, which the stage hook plans too: the samplers of engine_dit.hip are its only readers)
struct SampleWs {
    float *ts, *xt, *v, *x, *nz, *xt3, *v3;
    void plan(Bump& b, int B, int N, int n_steps, int cfg) {
        const size_t e = (size_t)B * N * kLatent;
        ts = b.take<float>(n_steps);
        xt = b.take<float>(e);
        v = b.take<float>(e);
        x = b.take<float>(e);
        nz = b.take<float>(e);
        xt3 = b.take<float>(cfg ? 3 * e : 1);
        v3 = b.take<float>(cfg ? 3 * e : 1);
    }
};
// THE workspace of a DiT operator, three parts: sampler buffers (n_steps > 0: sample) + modulation chain, table and LN-fold tables |
// core | cross-KV images of all 12 layers (Kc, Vc^T, each hi + lo).  B: the caller's rows, the evaluations run on 3B rows with cfg.
// A part is sized like every workspace of this file, its last offset + 256 bytes of slack (the cross part: + 256 per image as well); the
// core starts on the first 256-byte boundary behind the tables, the cross images behind the core and its slack.  plan() on a null base
// sizes (dit_ws_bytes), the same plan() on the workspace carves.
struct Engine::DitWs {
    SampleWs s;
    ModWs m;
    CoreWs core;
    CrossImg cross;
    size_t plan(void* base, int B, int N, int R, int P, int mod_rows, bool fold, int n_steps, int cfg) {
        auto behind = [](const Bump& b, size_t slack) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(b.p) + b.off + slack + 255) & ~uintptr_t(255)); };
        Bump tb(base);
        if (n_steps > 0) s.plan(tb, B, N, n_steps, cfg);
        m.plan(tb, mod_rows, fold);
        const int Bd = cfg ? 3 * B : B;
        Bump cb(behind(tb, 0));
        core.plan(cb, Bd, N);
        cross.Rp = pad8(R > 0 ? R : 0);
        cross.Cp = cross.Rp + pad8(P > 0 ? P : 0);
        const size_t n = (size_t)kBlocks * Bd * kHeads * cross.Cp * 128;
        Bump xb(behind(cb, 256));
        cross.kc = xb.take<bf16_t>(n); cross.kc_lo = xb.take<bf16_t>(n);
        cross.vtc = xb.take<bf16_t>(n); cross.vtc_lo = xb.take<bf16_t>(n);
        return (tb.off + 256) + (cb.off + 256) + (4 * (n * sizeof(bf16_t) + 256) + 256);
    }
};

// Workspace of one codec call.  Every caller plans it through codec_plan() for the WHOLE call the work belongs to: the gates of
// codec_block, conv_small_m and the resampling paths read the plan's sizes, so a part of a call (smtts_test_codec_stage) runs the
// kernels of the whole call only if it plans the same way.
struct Engine::CodecWs {
    float *xa, *xb, *nb, *lat;
    bf16_t *n2hi, *n2lo, *hhi, *hlo;
    size_t max_img, max_hid;
    void plan(Bump& b, const CodecPlan& p) {
        max_img = p.max_img;
        max_hid = p.max_hid;
        xa = b.take<float>(p.max_img);
        xb = b.take<float>(p.max_img);
        nb = b.take<float>(p.max_img);
        n2hi = b.take<bf16_t>(p.max_img);
        n2lo = b.take<bf16_t>(p.max_img);
        hhi = b.take<bf16_t>(p.max_hid);
        hlo = b.take<bf16_t>(p.max_hid);
        lat = b.take<float>(p.lat);
    }
};
