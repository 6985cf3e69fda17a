// Engine, test hooks and bench_gemm: single stages of the product's own code paths, and GEMMs on operands packed for the call.
#include "engine_impl.hpp"

namespace {
// The private device buffers of one hook call: owned here, freed when the hook returns, on whichever path.  A failed allocation
// returns null and stays in `err` (the later take()s still run: one check behind the last of them covers all).
struct Scratch {
    std::vector<void*> bufs;
    hipError_t err = hipSuccess;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { (void)release(); }
    template <class T>
    T* take(size_t n) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess) bufs.push_back(p);
        else if (err == hipSuccess) err = e;
        return static_cast<T*>(p);
    }
    hipError_t release() {   // (for a hook that reports a failed free)
        hipError_t first = hipSuccess;
        for (void* p : bufs) {
            const hipError_t e = hipFree(p);
            if (first == hipSuccess) first = e;
        }
        bufs.clear();
        return first;
    }
};
}  // namespace

// one codec stage (or a run of the pipeline's parts at one stage) through the functions above, on a workspace planned for the
// smallest whole call that contains this stage geometry: what that call's dispatch would run on these frames, this runs
int Engine::test_codec_stage(hipStream_t st, int part, int stage, int what, const float* xin, int B, int T_in, int C_in, float* out,
                             int* T_out, int* C_out) {
    if (part != 1 && part != 2) return fail("test_codec_stage: part must be 1 (decoder) or 2 (encoder)");
    const bool dec = part == 1;
    const CodecHalfW& h = dec ? dec_ : enc_;
    if (!h.ready) return fail("test_codec_stage: codec half not finalized");
    const CodecSpecC& s = cspec_;
    const int S = s.n_ratios + 1, pad = kCodecPad;
    if (stage < 0 || stage >= S) return fail("test_codec_stage: stage out of range");
    // the parts in pipeline order: stem (stage 0) or resampling (stage > 0), blocks, head (last stage); set bits must be a contiguous run
    const int seq[3] = {stage == 0 ? 1 : 2, 4, 8};
    if (what <= 0 || (what & ~(seq[0] | 4 | 8))) return fail("test_codec_stage: `what` names a part this stage does not have");
    {
        int first = -1, last = -1;
        for (int k = 0; k < 3; ++k)
            if (what & seq[k]) { if (first < 0) first = k; last = k; }
        for (int k = first; k <= last; ++k)
            if (!(what & seq[k])) return fail("test_codec_stage: `what` bits are not a run in pipeline order");
    }
    if ((what & 8) && stage != S - 1) return fail("test_codec_stage: the head belongs to the last stage");
    if (B <= 0 || T_in <= 0) return fail("test_codec_stage: B * T must be positive");
    // input geometry and the whole call (T0: decoder latent frames / encoder samples) whose plan this stage runs under
    const int r = stage > 0 ? h.stages[stage].r : 1;
    const int c_need = (what & 1) ? (dec ? s.latent_dim : 1) : (what & 2) ? h.stages[stage - 1].C : h.stages[stage].C;
    if (C_in != c_need) return fail("test_codec_stage: C_in " + std::to_string(C_in) + " does not match the stage (" + std::to_string(c_need) + ")");
    if (!dec && (what & 2) && T_in % r) return fail("test_codec_stage: encoder T_in must be a multiple of the stage's stride");
    const long Ts = (what & 2) ? (dec ? (long)T_in * r : T_in / r) : T_in;   // frames of the stage
    long up = 1;   // frames of the stage per decoder latent frame / encoder samples per frame of the stage
    for (int i = 1; i <= stage; ++i) up *= dec ? s.ratios[i - 1] : s.ratios[s.n_ratios - i];
    const long T0 = dec ? (Ts + up - 1) / up : Ts * up;
    if (T0 > (1L << 30) || Ts > (1L << 30)) return fail("test_codec_stage: too many frames");
    const int Cs = h.stages[stage].C;
    if (T_out) *T_out = (int)Ts;
    if (C_out) *C_out = (what & 8) ? (dec ? 1 : s.latent_dim) : Cs;
    if (!out) return 0;   // shape query
    if (!xin) return fail("test_codec_stage: null input");

    HIPC(hipSetDevice(device_));
    const CodecPlan plan = codec_plan(dec, B, T0);
    const size_t bytes = codec_ws_bytes(plan);
    Scratch scratch;
    void* const ws = scratch.take<char>(bytes);
    if (!ws) return fail_hip(scratch.err, "hipMalloc(&ws, bytes)");
    int rc = 0;
    {
        Bump bump(ws);
        CodecWs w;
        w.plan(bump, plan);
        float* x = w.xa;
        float* xn = w.xb;
        int Ti = T_in, C = c_need;
        auto run = [&]() -> int {
            // all-ones bytes: NaN in every operand format (fp32, bf16, fp16).  The product never clears its workspace (it zeroes the
            // causal pads itself); a kernel that read rows nobody wrote would turn this into NaN in the output instead of going unseen
            HIPC(hipMemsetAsync(ws, 0xff, bytes, st));
            if (what & 1) {
                if (dec ? decode_stem(st, w, xin, B, T_in) : encode_stem(st, w, xin, B, T_in)) return 1;
                C = Cs;
            } else {   // the input as the image the previous part would have left: zero causal pads, data rows
                HIPC(launch_zero_pad_frames3(x, xn, w.nb, B, Ti, C, pad, st));
                HIPC(hipMemcpy2DAsync(x + (long)pad * C, (size_t)(pad + Ti) * C * 4, xin, (size_t)Ti * C * 4, (size_t)Ti * C * 4, B,
                                      hipMemcpyDeviceToDevice, st));
            }
            if (what & (2 | 4))
                if (dec ? decode_stage(st, w, stage, what, &x, &xn, B, &Ti, &C) : encode_stage(st, w, stage, what, &x, &xn, B, &Ti, &C))
                    return 1;
            if (what & 8) return dec ? decode_head(st, w, x, B, Ti, C, out) : encode_head(st, w, x, B, Ti, C, out);
            HIPC(hipMemcpy2DAsync(out, (size_t)Ti * C * 4, x + (long)pad * C, (size_t)(pad + Ti) * C * 4, (size_t)Ti * C * 4, B,
                                  hipMemcpyDeviceToDevice, st));
            return 0;
        };
        rc = run();
    }
    const hipError_t es = hipStreamSynchronize(st);
    const hipError_t ef = scratch.release();
    if (rc) return rc;
    if (es != hipSuccess) return fail_hip(es, "test_codec_stage: stream");
    if (ef != hipSuccess) return fail_hip(ef, "test_codec_stage: free");
    return 0;
}

// Every launch of one scorer call, tapped (include/smalltts_hip.h smtts_test_scorer_taps): the product's own launcher with a tap sink, on
// a workspace of the product's own size function filled with 0xff first.  The size of the tap buffer (0 when refused); off (one entry
// per slot, or NULL) receives the byte offset of every slot.
size_t Engine::test_scorer_tap_bytes(int net, int B, int N, size_t* off, int cap) {
    if (net < 0 || net > 1) { fail("test_scorer_tap_bytes: net must be 0 (recogniser) or 1 (speaker verifier)"); return 0; }
    if (B < 1 || B > 64 || N < (net ? 6 : 1) || N > 225) {
        fail(std::string("test_scorer_tap_bytes: B must be in [1, 64] and N in [") + (net ? "6" : "1") + ", 225]");
        return 0;
    }
    const int n = net ? SV_TAPS : ASR_TAPS;
    if (off && cap < n) { fail("test_scorer_tap_bytes: the offset table needs one entry per slot"); return 0; }
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (off) off[i] = at;
        at += ((net ? sv_tap_bytes(B, N, i) : asr_tap_bytes(B, N, i)) + 255) & ~size_t(255);
    }
    return at;
}

int Engine::test_scorer_taps(hipStream_t st, int net, const float* x, const int32_t* n_len, int B, int N, float* out, void* taps,
                             size_t tap_bytes) {
    if (net < 0 || net > 1) return fail("test_scorer_taps: net must be 0 (recogniser) or 1 (speaker verifier)");
    size_t (*const need)(int, int) = net ? sv_ws_bytes : asr_ws_bytes;
    // what the entry itself refuses; the workspace is this hook's own (checked as an aligned one of the size the entry asks for)
    void* const aligned = reinterpret_cast<void*>(uintptr_t(256));
    if (net ? scorer_entry("test_scorer_taps", "sv", "speaker verifier", "emb", sv_ready_, 6, need, x, n_len, B, N, aligned, need(B < 1 ? 1 : B, N < 6 ? 6 : N), out)
            : scorer_entry("test_scorer_taps", "asr", "recogniser", "logp", asr_ready_, 1, need, x, n_len, B, N, aligned, need(B < 1 ? 1 : B, N < 1 ? 1 : N), out))
        return 1;
    size_t off[ASR_TAPS];
    static_assert(SV_TAPS <= ASR_TAPS, "off[] holds either table");
    const size_t need_taps = test_scorer_tap_bytes(net, B, N, off, ASR_TAPS);
    if (!need_taps) return 1;
    if (!taps) return fail("smtts_test_scorer_taps: a required pointer is NULL");
    if ((uintptr_t)taps & 255) return fail("smtts_test_scorer_taps: the tap buffer must be 256-byte aligned");
    if (tap_bytes < need_taps) return fail("smtts_test_scorer_taps: tap buffer too small (smtts_test_scorer_tap_bytes)");
    HIPC(hipSetDevice(device_));
    const size_t bytes = need(B, N);
    Scratch scratch;
    void* const ws = scratch.take<char>(bytes);
    if (!ws) return fail_hip(scratch.err, "hipMalloc(&ws, bytes)");
    hipError_t e = hipMemsetAsync(ws, 0xff, bytes, st);   // NaN: a launch that read what nobody wrote shows up in its tap
    if (e == hipSuccess) {
        ProfTag tag(net ? "sv" : "asr");
        const ScorerTaps sink{static_cast<char*>(taps), off};
        e = net ? launch_sv_embed(sv_, x, n_len, B, N, ws, out, st, &sink) : launch_asr_logprobs(asr_, x, n_len, B, N, ws, out, st, &sink);
    }
    const hipError_t es = hipStreamSynchronize(st);
    const hipError_t ef = scratch.release();
    if (e != hipSuccess) return fail_hip(e, "test_scorer_taps");
    if (es != hipSuccess) return fail_hip(es, "test_scorer_taps: stream");
    if (ef != hipSuccess) return fail_hip(ef, "test_scorer_taps: free");
    return 0;
}

// DiT / encoder stages through the code of denoise_step / sample / cond_encode (include/smalltts_hip.h smtts_test_dit_stage).  The
// workspace is planned by the product's own planners (DitWs, EncWs) and filled with 0xff first.
int Engine::test_dit_stage(hipStream_t st, int net, int what, int l0, int l1, int path, int twice, const void* xin,
                           const uint8_t* mask, int B, int S, const float* t, const float* modin, int mod_rows, int mod_row0,
                           int mod_rstride, const float* k_ref, const float* v_ref, const uint8_t* ref_mask, int R,
                           const float* k_text, const float* v_text, const uint8_t* ph_mask, int P, const float* rope,
                           float* x_out, float* img_out, float* shift_out, float* out, float* k_out, float* v_out, float* mod_out) {
    if (!dit_ready_) return fail("test_dit_stage: DiT weights not finalized");
    if (net < 0 || net > 2) return fail("test_dit_stage: net must be 0 (DiT), 1 (style encoder) or 2 (text encoder)");
    if (what <= 0 || what > 15) return fail("test_dit_stage: `what` must be a non-empty set of the bits 1, 2, 4, 8");
    if (path < 0 || path > 3) return fail("test_dit_stage: path must be 0 (the operator's choice), 1 (fold), 2 (split-K) or 3 (unsplit)");
    if (B <= 0 || S <= 0) return fail("test_dit_stage: B and S must be positive");
    if (S > kMaxPos) return fail("test_dit_stage: sequence longer than the rope table (4096)");
    if ((long)B * S > (1L << 20)) return fail("test_dit_stage: too many rows");
    const bool dit = net == 0;
    const EncoderW* enc = net == 1 ? &style_ : net == 2 ? &text_ : nullptr;
    const int L = dit ? kBlocks : (int)enc->blocks.size(), M = B * S, D = dit ? kHidden : enc->dim;
    // the chain bits (DiT: 2 embed, 4 blocks, 8 head; mod = bit 1 rides along.  Encoders: 1 in, 2 blocks, 4 out, 8 kv) form a run
    const int chain = dit ? what & 14 : what;
    {
        int first = -1, last = -1;
        for (int k = 0; k < 4; ++k)
            if (chain & (1 << k)) { if (first < 0) first = k; last = k; }
        for (int k = first; first >= 0 && k <= last; ++k)
            if (!(chain & (1 << k))) return fail("test_dit_stage: `what` bits are not a run in pipeline order");
    }
    const int BLK = dit ? 4 : 2, FIRST = dit ? 2 : 1, AFTER = dit ? 8 : 4;
    const bool blocks = (what & BLK) != 0;
    if (blocks && (l0 < 0 || l0 >= l1 || l1 > L)) return fail("test_dit_stage: block range [l0, l1) outside [0, " + std::to_string(L) + ")");
    if (blocks && (what & FIRST) && l0 != 0) return fail("test_dit_stage: the input stage feeds block 0 only");
    if (blocks && (what & AFTER) && l1 != L) return fail("test_dit_stage: the stage after the blocks reads the last block's output only");
    if (R < 0 || P < 0 || R > kMaxPos || P > kMaxPos) return fail("test_dit_stage: R / P outside [0, 4096]");
    if (!xin && chain) return fail("test_dit_stage: null input");
    // the path of the block stage: what the product runs on this call (0), or one of its paths, refused where the product never takes it
    bool fold = false;
    int ks = 1;
    const int ks_dit = tuning_ == TUNE_THROUGHPUT || M > 1024 ? 1 : ksplit_out_;   // (denoise_step's choice outside the fold)
    if (dit) {
        if (path == 1 && !dit_fold_on(M)) return fail("test_dit_stage: no LN-fold here (M > 1024, fold off, or no epilogue attention)");
        if (path == 1 && (mod_rstride != 0 || (what & BLK) == 0)) return fail("test_dit_stage: the fold runs blocks with one modulation row only");
        if (path == 2 && (M > 1024 || ksplit_out_ < 2)) return fail("test_dit_stage: no split-K at M > 1024");
        fold = path == 1;
        ks = path == 2 ? ksplit_out_ : path == 3 ? 1 : ks_dit;   // (the fold's last FF2 leaves it: the operator's choice there)
        if (what & (1 | 4)) {   // a modulation table: from t (bit 1) or the caller
            if (mod_rows <= 0 || mod_row0 < 0 || mod_rstride < 0 || mod_rstride > 1 || mod_row0 + (long)(B - 1) * mod_rstride >= mod_rows)
                return fail("test_dit_stage: modulation rows / row0 / stride do not cover the batch");
            if ((what & 1) ? !t : !modin) return fail("test_dit_stage: null t / modulation table");
        }
        if ((what & 4) && !mask) return fail("test_dit_stage: null mask");
        if ((what & 2) && !mask) return fail("test_dit_stage: null mask");
        if ((what & 4) && ((R > 0 && (!k_ref || !v_ref || !ref_mask)) || (P > 0 && (!k_text || !v_text || !ph_mask))))
            return fail("test_dit_stage: null cross cache / mask");
    } else {
        if (path == 1 && !(fold_epi_on() && D % 64 == 0)) return fail("test_dit_stage: no RMSNorm fold here");
        if (path == 2 && ksplit_enc_ < 2) return fail("test_dit_stage: split-K is off in this build");
        fold = path == 1 || (path == 0 && fold_epi_on() && D % 64 == 0);
        ks = path == 3 ? 1 : ksplit_enc_;
        if ((what & (2 | 4)) && !mask) return fail("test_dit_stage: null key mask");
    }
    if (!dit && (what & 8) && (!k_out || !v_out)) return fail("test_dit_stage: null K / V output");

    HIPC(hipSetDevice(device_));
    // workspace: as denoise_step / sample plan it (modulation table + LN-fold tables, core, cross images), or as cond_encode does
    const bool need_mod = dit && (what & (1 | 4));
    size_t bytes = dit ? dit_ws_bytes(B, S, R, P, need_mod ? mod_rows : 1, fold, 0, 0) : 0;
    if (!dit) {
        Bump b(nullptr);
        EncWs e;
        e.plan(b, B, S);
        bytes = b.off + 256;
    }
    Scratch scratch;
    void* const ws = scratch.take<char>(bytes);
    if (!ws) return fail_hip(scratch.err, "hipMalloc(&ws, bytes)");
    int rc = 0;
    {
        ProfTag ptag(dit ? "dit" : "enc");
        // all-ones bytes: NaN in every operand format; a kernel that read what nobody wrote would turn it into NaN in the output
        Call call(st);
        auto run = [&]() -> int {
            Bump bump(ws);
            if (dit) {
                DitWs dw;
                dw.plan(ws, B, S, R, P, need_mod ? mod_rows : 1, fold, 0, 0);
                const ModWs& m = dw.m;
                const CoreWs& w = dw.core;
                if (need_mod) {
                    if (what & 1) {
                        if (modulation(st, t, mod_rows, m)) return 1;
                    } else {
                        HIPC(hipMemcpyAsync(m.mod, modin, (size_t)mod_rows * kModLd * 4, hipMemcpyDeviceToDevice, st));
                        if (fold && fold_tables(st, m.mod, mod_rows, m.ftab)) return 1;
                    }
                    if (mod_out) HIPC(hipMemcpyAsync(mod_out, m.mod, (size_t)mod_rows * kModLd * 4, hipMemcpyDeviceToDevice, st));
                }
                if (what & 2) {
                    if (dit_embed(st, w, static_cast<const float*>(xin), mask, B, S, !call.ws_zeroed)) return 1;
                } else if (what & 4) {
                    HIPC(hipMemcpyAsync(w.x, xin, (size_t)M * kHidden * 4, hipMemcpyDeviceToDevice, st));
                }
                if (what & 4) {
                    Cond cond{k_ref, v_ref, k_text, v_text, ref_mask, ph_mask, R, P, {}};
                    if (pack_cross(st, cond, B, dw.cross)) return 1;
                    DitRun d;
                    if (dit_run(st, w, mask, ModRow{m.mod, mod_row0, mod_rstride, m.ftab}, cond, rope, B, S, fold, ks == 1, d)) return 1;
                    if (dit_blocks(st, w, d, l0, l1, call)) return 1;
                    const int pi = prec_[l1 == kBlocks ? SITE_COND : SITE_DIT_BLOCK];
                    if (img_out) {
                        const SplitBuf y = w.y.as(pi, nullptr);
                        HIPC(launch_split_to_f32(y.hi, y.lo, img_out, (long)M * kHidden, st));
                    }
                    if (shift_out) {
                        if (fold && LN_FOLD_SHIFT) HIPC(hipMemcpyAsync(shift_out, w.lnc, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
                        else HIPC(hipMemsetAsync(shift_out, 0, (size_t)M * 4, st));
                    }
                }
                if ((what & (2 | 4)) && x_out) HIPC(hipMemcpyAsync(x_out, w.x, (size_t)M * kHidden * 4, hipMemcpyDeviceToDevice, st));
                if (what & 8) {
                    if (!(what & 4)) {   // the input as the final AdaLN image the last block would have left (SITE_COND format)
                        const SplitBuf y = w.y.as(prec_[SITE_COND], nullptr);
                        HIPC(launch_to_split(static_cast<const float*>(xin), rowmap_plain(kHidden), y.hi, y.lo, rowmap_plain(kHidden), M,
                                             kHidden, st));
                    }
                    if (out && dit_head(st, w, M, out)) return 1;
                }
                return 0;
            }
            EncWs w;
            w.plan(bump, B, S);
            const bool text = net == 2;
            if (what & 1) {
                if (text ? text_in(st, w, static_cast<const int64_t*>(xin), B, S) : style_in(st, w, static_cast<const float*>(xin), B, S))
                    return 1;
            } else if (what & 2) {
                HIPC(hipMemcpyAsync(w.x, xin, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
            }
            if (what & 2) {
                if (enc_blocks(st, *enc, w, l0, l1, B, S, mask, fold, ks)) return 1;
                if (img_out) {
                    const SplitBuf y = w.y.as(prec_[SITE_ENCODER], nullptr);
                    HIPC(launch_split_to_f32(y.hi, y.lo, img_out, (long)M * D, st));
                }
            }
            if ((what & (1 | 2)) && x_out) HIPC(hipMemcpyAsync(x_out, w.x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
            float* seq = out ? out : w.seq;
            if (what & 4) {
                if (!(what & 2)) {   // the input as the final norm image (SITE_ENCODER format)
                    const SplitBuf y = w.y.as(prec_[SITE_ENCODER], nullptr);
                    HIPC(launch_to_split(static_cast<const float*>(xin), rowmap_plain(D), y.hi, y.lo, rowmap_plain(D), M, D, st));
                }
                if (enc_out(st, text, w, M, mask, seq)) return 1;
            }
            if (what & 8) {
                const float* src = (what & 4) ? seq : static_cast<const float*>(xin);
                if (enc_kv(st, text, w, src, B, S, k_out, v_out)) return 1;
            }
            return 0;
        };
        rc = hipMemsetAsync(ws, 0xff, bytes, st) != hipSuccess ? fail("test_dit_stage: memset") : run();
        // twice: a second run on the same workspace, as the sampler's later steps find it (its never-written regions are not zeroed again)
        call.ws_zeroed = true;
        if (!rc && twice) rc = run();
    }
    const hipError_t es = hipStreamSynchronize(st);
    const hipError_t ef = scratch.release();
    if (rc) return rc;
    if (es != hipSuccess) return fail_hip(es, "test_dit_stage: stream");
    if (ef != hipSuccess) return fail_hip(ef, "test_dit_stage: free");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// test hooks
// ---------------------------------------------------------------------------------------------
int Engine::test_gemm(hipStream_t st, const float* A, int lda, const float* W, const float* bias, int M, int N, int K,
                      int act, int split, int cfg, float* C, int ldc) {
    HIPC(hipSetDevice(device_));
    Scratch scratch;
    bf16_t* const hi = scratch.take<bf16_t>((size_t)N * K);
    bf16_t* const lo = scratch.take<bf16_t>((size_t)N * K);
    HIPC(scratch.err);
    HIPC(launch_split_rows(W, K, hi, lo, K, N, K, nullptr, st));
    PW w;
    w.hi = hi; w.lo = lo; w.N = N; w.K = K;
    hipError_t e = gemm_store(ops(A, rowmap_plain(lda), w, M), act, store_to(C, rowmap_plain(ldc), bias), 1, split, st, tune_, cfg);
    (void)hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : fail_hip(e, "test_gemm");
}

int Engine::test_gemm3(hipStream_t st, const float* A, const float* W, const float* bias, int M, int N, int K, int act,
                       int split, int cfg, float* C) {
    HIPC(hipSetDevice(device_));
    Scratch scratch;
    bf16_t* const hi = scratch.take<bf16_t>((size_t)N * K);
    bf16_t* const lo = scratch.take<bf16_t>((size_t)N * K);
    bf16_t* const ahi = scratch.take<bf16_t>((size_t)M * K);
    bf16_t* const alo = scratch.take<bf16_t>((size_t)M * K);
    HIPC(scratch.err);
    // PREC_F16: the single 16-bit arrays (hi) carry fp16
    HIPC(launch_split_rows(W, K, split == PREC_F16 ? nullptr : hi, lo, K, N, K, nullptr, st, split == PREC_F16 ? hi : nullptr));
    HIPC(launch_to_split(A, rowmap_plain(K), ahi, sm_lo_for(split, alo), rowmap_plain(K), M, K, st));
    PW w;
    w.hi = hi; w.lo = lo; w.h16 = hi; w.N = N; w.K = K;
    hipError_t e = gemm3_store(ops3(SplitBuf{ahi, alo}, rowmap_plain(K), w, M, split), act, store_to(C, rowmap_plain(N), bias), 1,
                               split, st, tune_, cfg);
    (void)hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : fail_hip(e, "test_gemm3");
}

// One LN-fold step of the real chain in isolation (gemm.hpp LnFoldIn): the producer (gated residual of x, operand image, row partials),
// the fold tables of ONE site from fold_vectors_kernel (LayerNorm only) and the SwiGLU consumer; fold = 0 runs the norm-launch path of
// the same step (plain residual, ln_modulate / rmsnorm, plain SwiGLU).  x [M][D] is updated in place; h [M][F] = the hidden image, decoded.
int Engine::test_ln_fold(hipStream_t st, const float* A, const float* Wp, const float* bp, const float* gate, const uint8_t* mask,
                         const float* nscale, const float* shift, const float* W1, const float* W3, const float* b1, const float* b3,
                         int M, int K, int D, int F, float eps, int rms, int prec, int fold, float* x, float* h, float* c_out) {
    HIPC(hipSetDevice(device_));
    if (M <= 0 || K % 64 || D % 32 || F % 32 || F <= 0) return fail("test_ln_fold: M > 0, K % 64 == 0, D % 32 == 0, F % 32 == 0");
    if (prec != PREC_BF16 && prec != PREC_F16 && prec != PREC_BF16X3) return fail("test_ln_fold: precision must be 1, 2 or 3");
    if (!nscale || (!rms && !shift)) return fail("test_ln_fold: scale (and, for LayerNorm, shift) required");
    if (fold && (D / 32) % 2) return fail("test_ln_fold: LN-fold needs an even number of 32-column partial groups (D % 64 == 0)");
    if (fold && !rms && D != kHidden) return fail("test_ln_fold: the fold-table kernel multiplies K = 960 weights");
    const int NP = D / 32;
    const bool f16 = prec == PREC_F16;
    Scratch scratch;
    bf16_t* const wp_hi = scratch.take<bf16_t>((size_t)D * K);
    bf16_t* const wp_lo = scratch.take<bf16_t>((size_t)D * K);
    bf16_t* const w13_hi = scratch.take<bf16_t>((size_t)2 * F * D);
    bf16_t* const w13_lo = scratch.take<bf16_t>((size_t)2 * F * D);
    float* const cat = scratch.take<float>((size_t)2 * F * D);
    std::vector<int> perm = swiglu_perm(F);
    int* const dperm = scratch.take<int>(perm.size());
    bf16_t* const a_hi = scratch.take<bf16_t>((size_t)M * K);
    bf16_t* const a_lo = scratch.take<bf16_t>((size_t)M * K);
    bf16_t* const y_hi = scratch.take<bf16_t>((size_t)M * D);
    bf16_t* const y_lo = scratch.take<bf16_t>((size_t)M * D);
    bf16_t* const f_hi = scratch.take<bf16_t>((size_t)M * F);
    bf16_t* const f_lo = scratch.take<bf16_t>((size_t)M * F);
    float* const part = scratch.take<float>((size_t)M * NP * 2);
    float* const modrow = scratch.take<float>((size_t)2 * D);
    float* const tab = scratch.take<float>((size_t)2 * 2 * F);
    float* const cs = scratch.take<float>((size_t)M);
    HIPC(scratch.err);
    HIPC(launch_split_rows(Wp, K, f16 ? nullptr : wp_hi, wp_lo, K, D, K, nullptr, st, f16 ? wp_hi : nullptr));
    HIPC(hipMemcpyAsync(cat, W1, (size_t)F * D * 4, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(cat + (size_t)F * D, W3, (size_t)F * D * 4, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(dperm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPC(launch_split_rows(cat, D, f16 ? nullptr : w13_hi, w13_lo, D, 2 * F, D, dperm, st, f16 ? w13_hi : nullptr));
    HIPC(launch_to_split(A, rowmap_plain(K), a_hi, sm_lo_for(prec, a_lo), rowmap_plain(K), M, K, st));
    PW wp, w13;
    wp.hi = wp.h16 = wp_hi; wp.lo = wp_lo; wp.N = D; wp.K = K;
    w13.hi = w13.h16 = w13_hi; w13.lo = w13_lo; w13.N = 2 * F; w13.K = D;
    const RowMap rd = rowmap_plain(D);
    const SplitBuf y = SplitBuf{y_hi, y_lo}.as(prec), ffh = SplitBuf{f_hi, f_lo}.as(prec);
    EpiSwiGLU sw{nullptr, F, b1, b3, ffh.hi, ffh.lo};
    if (fold) {
        if (!rms) {   // the tables of one site: W shift and W (1 + scale) on the weights the consumer multiplies
            HIPC(hipMemcpyAsync(modrow, shift, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
            HIPC(hipMemcpyAsync(modrow + D, nscale, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
            FoldSites fs{};
            fs.n = 1;
            fs.NF = 2 * F;
            FoldSite& f = fs.s[0];
            f.w = w13_hi; f.wlo = prec == PREC_BF16X3 ? w13_lo : nullptr; f.fmt = f16 ? 0 : 1; f.N = 2 * F;
            f.shift_off = 0; f.scale_off = D; f.out_off = 0;
            HIPC(launch_fold_vectors(fs, modrow, 2 * D, 1, tab, st));
            // the row shift as the chain has it in front of its first producer: the mean ln_modulate took of x (its image is
            // overwritten by the producer)
            if (LN_FOLD_SHIFT) HIPC(launch_ln_modulate(x, nullptr, y.hi, y.lo, M, D, eps, shift, nscale, 0, 0, 0, M, st, cs));
        }
        float* const csh = !rms && LN_FOLD_SHIFT ? cs : nullptr;
        EpiResidLN p{x, rd, bp, gate, mask, nscale, y.hi, y.lo, D, part, NP, rms, csh};
        HIPC(gemm3_resid_ln(ops3(SplitBuf{a_hi, a_lo}, rowmap_plain(K), wp, M, prec), p, prec, st, tune_));
        LnFoldIn fin;
        fin.part = part; fin.NP = NP; fin.inv_c = 1.0f / D; fin.eps = eps; fin.rms = rms;
        if (!rms) { fin.wsh = tab; fin.wc = tab + 2 * F; fin.cshift = csh; fin.nh = F; }
        sw.fold = fin;
    } else {
        EpiResid<0> r{x, rd, bp, gate, 0, 0, 0, M, mask};
        HIPC(gemm3_resid(ops3(SplitBuf{a_hi, a_lo}, rowmap_plain(K), wp, M, prec), gate ? 2 : 0, r, prec, st, tune_));
        if (rms) {
            HIPC(launch_rmsnorm(x, rd, nullptr, y.hi, y.lo, rd, M, D, eps, nscale, st));
        } else {
            HIPC(launch_ln_modulate(x, nullptr, y.hi, y.lo, M, D, eps, shift, nscale, 0, 0, 0, M, st));
        }
    }
    HIPC(gemm3_swiglu(ops3(y, rd, w13, M, prec), sw, prec, st, tune_));
    HIPC(launch_split_to_f32(ffh.hi, ffh.lo, h, (long)M * F, st));
    if (c_out) {   // the row shift as the consumer left it for the next producer (0 where the step has none)
        if (sw.fold.cshift) HIPC(hipMemcpyAsync(c_out, sw.fold.cshift, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
        else HIPC(hipMemsetAsync(c_out, 0, (size_t)M * 4, st));
    }
    (void)hipStreamSynchronize(st);
    return 0;
}

int Engine::test_swiglu(hipStream_t st, const float* A, const float* W1, const float* W3, const float* b1,
                        const float* b3, int M, int F, int K, int split, float* out) {
    HIPC(hipSetDevice(device_));
    if (F % 32) return fail("test_swiglu: F must be a multiple of 32");
    std::vector<int> perm = swiglu_perm(F);
    Scratch scratch;
    float* const cat = scratch.take<float>((size_t)2 * F * K);
    int* const dperm = scratch.take<int>(perm.size());
    bf16_t* const hi = scratch.take<bf16_t>((size_t)2 * F * K);
    bf16_t* const lo = scratch.take<bf16_t>((size_t)2 * F * K);
    HIPC(scratch.err);
    HIPC(hipMemcpyAsync(cat, W1, (size_t)F * K * 4, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(cat + (size_t)F * K, W3, (size_t)F * K * 4, hipMemcpyDeviceToDevice, st));
    HIPC(hipMemcpyAsync(dperm, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPC(launch_split_rows(cat, K, hi, lo, K, 2 * F, K, dperm, st));
    PW w;
    w.hi = hi; w.lo = lo; w.N = 2 * F; w.K = K;
    EpiSwiGLU sw{out, F, b1, b3, nullptr, nullptr};
#ifdef SMTTS_TEST_KERNELS
    hipError_t e = gemm_swiglu(ops(A, rowmap_plain(K), w, M), sw, split, st, tune_);
#else
    hipError_t e = hipErrorNotSupported;   // (the v1 SwiGLU instantiations are test kernels: make TEST_KERNELS=1)
#endif
    (void)hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : fail_hip(e, "test_swiglu");
}

// epi: 0 store, 1 store+gelu, 2 swiglu (N = packed 2F), 3 resid tanh-gate
int Engine::bench_gemm(int M, int N, int K, int epi, int split, int cfg, int iters, int ver, float* avg_us) {
    HIPC(hipSetDevice(device_));
    Scratch scratch;
    bf16_t* const ahi = scratch.take<bf16_t>((size_t)M * K);
    bf16_t* const alo = scratch.take<bf16_t>((size_t)M * K);
    float* const A = scratch.take<float>((size_t)M * K);
    float* const Wf = scratch.take<float>((size_t)N * K);
    float* const C = scratch.take<float>((size_t)M * N);
    float* const bias = scratch.take<float>((size_t)N);
    float* const gate = scratch.take<float>((size_t)N);
    bf16_t* const hi = scratch.take<bf16_t>((size_t)N * K);
    bf16_t* const lo = scratch.take<bf16_t>((size_t)N * K);
    uint8_t* const maskb = scratch.take<uint8_t>((size_t)M);
    bf16_t* const yimg = scratch.take<bf16_t>((size_t)M * N);
    float* const partb = scratch.take<float>((size_t)M * ((N + 31) / 32) * 2);
    HIPC(scratch.err);
    HIPC(hipMemset(maskb, 1, (size_t)M));
    HIPC(launch_synth(A, (long)M * K, 1, 0.f, 1.f, 0));
    HIPC(launch_synth(Wf, (long)N * K, 2, 0.f, 0.05f, 0));
    HIPC(launch_synth(bias, N, 3, 0.f, 0.1f, 0));
    HIPC(launch_synth(gate, N, 4, 0.f, 0.5f, 0));
    HIPC(hipMemsetAsync(C, 0, (size_t)M * N * 4, 0));
    HIPC(launch_split_rows(Wf, K, split == PREC_F16 ? nullptr : hi, lo, K, N, K, nullptr, 0, split == PREC_F16 ? hi : nullptr));
    PW w;
    w.hi = hi; w.lo = lo; w.h16 = hi; w.N = N; w.K = K;
    GemmOperands g = ops(A, rowmap_plain(K), w, M);
    HIPC(launch_to_split(A, rowmap_plain(K), ahi, sm_lo_for(split, alo), rowmap_plain(K), M, K, 0));
    Gemm3Operands g3 = ops3(SplitBuf{ahi, alo}, rowmap_plain(K), w, M, split);
    auto run = [&]() -> hipError_t {
        if (ver == 3) {
            switch (epi) {
                case 0: return gemm3_store(g3, ACT_NONE, store_to(C, rowmap_plain(N), bias), 1, split, 0, tune_, cfg);
                case 1: return gemm3_store(g3, ACT_GELU, store_to(C, rowmap_plain(N), bias), 1, split, 0, tune_, cfg);
                case 2: { EpiSwiGLU sw{C, N / 2, bias, bias, nullptr, nullptr}; return gemm3_swiglu(g3, sw, split, 0, tune_); }
                case 4: {   // GELU hidden written as ONE 16-bit operand array (the codec's first FFN product): C is reused as that array
                    EpiStore<ACT_NONE> e{nullptr, rowmap_plain(N), 0, bias, 0, 1.f, nullptr, reinterpret_cast<bf16_t*>(C), sm_lo_for(split == PREC_BF16X3 ? PREC_F16 : split, nullptr)};
                    return gemm3_store(g3, ACT_GELU, e, 1, split, 0, tune_, cfg);
                }
                case 5: { EpiResid<0> r{C, rowmap_plain(N), bias, gate, 0, 0, 0, M, nullptr}; return gemm3_resid(g3, 2, r, split, 0, tune_, cfg); }   // LayerScale residual (codec FF2)
                case 6: return gemm3_store(g3, ACT_NONE, store_to(C, rowmap_plain(N), nullptr), 1, split, 0, tune_, cfg);   // no bias: what a split-K slice stores
                case 7: case 9: {   // LN-fold producer (the DiT's out-proj with a row mask / FF2 without): residual + next operand image + row partials
                    EpiResidLN r{C, rowmap_plain(N), bias, gate, epi == 7 ? maskb : nullptr, bias, yimg, sm_lo_for(split == PREC_BF16X3 ? PREC_F16 : split, nullptr), N, partb, N / 32};
                    return gemm3_resid_ln(g3, r, split, 0, tune_, cfg);
                }
                case 8: { EpiResid<0> r{C, rowmap_plain(N), bias, gate, 0, 0, 0, M, maskb}; return gemm3_resid(g3, 1, r, split, 0, tune_, cfg); }   // tanh-gated residual with a row mask
                default: { EpiResid<0> r{C, rowmap_plain(N), bias, gate, 0, 0, 0, M, nullptr}; return gemm3_resid(g3, 1, r, split, 0, tune_, cfg); }
            }
        }
        switch (epi) {
            case 0: return gemm_store(g, ACT_NONE, store_to(C, rowmap_plain(N), bias), 1, split, 0, tune_, cfg);
            case 1: return gemm_store(g, ACT_GELU, store_to(C, rowmap_plain(N), bias), 1, split, 0, tune_, cfg);
#ifdef SMTTS_TEST_KERNELS
            case 2: { EpiSwiGLU sw{C, N / 2, bias, bias, nullptr, nullptr}; return gemm_swiglu(g, sw, split, 0, tune_); }
#endif
            default: { EpiResid<0> r{C, rowmap_plain(N), bias, gate, 0, 0, 0, M, nullptr}; return gemm_resid(g, 1, r, split, 0, tune_, cfg); }
        }
    };
    for (int i = 0; i < 3; ++i) HIPC(run());
    hipEvent_t e0, e1;
    HIPC(hipEventCreate(&e0));
    HIPC(hipEventCreate(&e1));
    HIPC(hipEventRecord(e0, 0));
    for (int i = 0; i < iters; ++i) HIPC(run());
    HIPC(hipEventRecord(e1, 0));
    HIPC(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}
