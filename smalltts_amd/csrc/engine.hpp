// smalltts gfx950 engine: owns the weights (fp32 originals + bf16 hi/lo GEMM packs) for one GPU and
// sequences the kernels of the three boundary operators the reference runs through onnxruntime
// (condition_encoder / denoiser / codec, reference infer/onnx.py:91-128) plus the fused sampler.
// One Engine per GPU, driven by one host thread (mirrors the reference's one-Session-per-pipeline model, src/server/src/main.rs:24).
// That thread may keep several operator calls in flight on DIFFERENT streams as long as each call has its own workspace and outputs:
// what belongs to one call lives in that call — its device scratch (incl. the rope cos / sin of a caller-supplied table) in the
// workspace, its host state (side set, owed join, zeroed workspace regions, text-attention tap) in the Call record the operator
// entry creates and hands down.  The engine keeps configuration, the weights (read-only after finalize()), the map of side sets
// (the dual-stream condition encoder / modulation chain forks onto a side stream that belongs to the CALLER's stream, one per caller
// stream), the error string and the profiler — and is not thread-safe because of the last three.  Per-kernel profiling assumes one
// call at a time.
#pragma once
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "gemm_ops.hpp"
#include "kernels.hpp"
#include "prof.hpp"

struct RawTensor {
    float* d = nullptr;
    std::vector<long> shape;
    long numel = 0;
};

struct PW {  // packed GEMM weight [N][K]: bf16 hi + lo (PREC_BF16X3 / PREC_BF16) and the same rows as fp16 (PREC_F16)
    bf16_t* hi = nullptr;
    bf16_t* lo = nullptr;
    bf16_t* h16 = nullptr;
    bf16_t* l16 = nullptr;   // fp16(w - float(h16)): only where PREC_F16X2 can run (the codec decoder's ConvTranspose weights)
    int N = 0, K = 0;  // K = row stride = GEMM K (may be zero-padded beyond the source width)
};

struct EncBlockW {
    PW qkvg, wo, ff13, w2;
    const float *qn, *kn, *an, *mn;
};
struct EncoderW {
    int dim, heads, dh, ff, layers;
    float eps;
    std::vector<EncBlockW> blocks;
    const float* final_norm;
    float* rope_cos;  // [MAXPOS][dh] cos / sin of pos * theta^(-2i/dh)
    float* rope_sin;
};
struct DitBlockW {
    std::string name;  // tensor-name prefix of the block ("dit.transformer_blocks.<i>")
    PW qkvg;           // [to_q; to_k_self; to_v_self; gate] unpadded (3840 x 960): only the A/B paths read it (SMTTS_ATTN_IMG=0 / SMTTS_ATTN_EPI=0,
                       // smtts_test_set_attention_mfma) — built on first use (Engine::ensure_qkvg_unpadded), N == 0 until then: 280 MB less resident
    PW out, ff13, ff2;
    PW qkvgp;          // the same rows with every head padded 120 -> 128 (zero rows): [4 x 8 x 128][960], gemm3 EpiQKV's column layout
    float* b_qkvgp;    // bias in that layout (pad and gate entries zero)
    float* b_qkvg;
    const float *b1, *b3, *b2, *qn, *kn;
};
struct CodecBlockW {
    const float *norm_w, *dw_b, *gamma, *ffn_norm_w, *b1, *b2, *ffn_gamma;
    float* dw_w;  // [K][C]
    PW w1, w2;
    PW w2t;       // C = 128 / 256: W2 repacked hidden-tile-major [F/32][C][32] for codec_ffn_stream.hip; N == 0 when unused
    bool f16_ok = true;   // the fused FFN kernels' hidden / input range is certified inside fp16 (Engine::certify_codec_ffn); false:
                          // this block's FFN runs split-bf16 whatever the site precision says (those kernels convert WITHOUT clamping)
};
struct CodecStageW {
    int C = 0, r = 0;  // r: resample ratio entering this stage (0 for stage 0)
    PW resample;       // decoder: ConvTranspose as GEMM [r*C][2*Cprev]; encoder: strided conv [C][2r*Cprev]
    float* resample_bias = nullptr;
    std::vector<CodecBlockW> blocks;
};
struct CodecHalfW {
    bool ready = false;
    std::vector<CodecStageW> stages;
    PW stem;                 // decoder: [C0][K*latent]   (encoder stem is a direct 1-channel conv)
    const float* stem_b = nullptr;
    const float* stem_w_raw = nullptr;  // encoder
    PW head;                 // encoder: [latent][K*Clast]
    float* head_w = nullptr; // decoder: [K][Clast] fp32
    float head_b_host = 0.f;
    const float* head_b = nullptr;
    const float* final_norm_w = nullptr;  // optional RMSNorm in front of the head conv
};

struct CodecSpecC {
    int latent_dim = 64, n_filters = 32, kernel = 7, ffn_mult = 4, n_ratios = 6;
    int ratios[8] = {8, 5, 5, 4, 2, 2, 0, 0};   // decoder order
    int depths[9] = {8, 3, 3, 3, 3, 3, 3, 0, 0};  // decoder order, n_ratios + 1 entries
    float eps = 1e-5f;
    int hop() const { int h = 1; for (int i = 0; i < n_ratios; ++i) h *= ratios[i]; return h; }
};

static constexpr int kDefaultPrecision = PREC_F16;   // "f16 mixed" (DESIGN §2): one default for the C ABI and the Python host side

class Engine {
  public:
    explicit Engine(int device);
    ~Engine();
    int device() const { return device_; }
    const std::string& last_error() const { return err_; }

    // ---- weights ---------------------------------------------------------------------------
    int set_tensor(const char* name, const float* data, const long* shape, int ndim, bool src_on_device);
    int synth_tensor(const char* name, const long* shape, int ndim, uint64_t key, float mean, float half_range);
    int get_tensor(const char* name, float* host_out, long numel);
    int set_codec_spec(const CodecSpecC& s);
    int finalize();  // build GEMM packs for whatever model parts are present
    bool has_dit() const { return dit_ready_; }
    bool has_decoder() const { return dec_.ready; }
    bool has_encoder() const { return enc_.ready; }
    bool has_asr() const { return asr_ready_; }
    bool has_sv() const { return sv_ready_; }
    // Per-site operand precision (PREC_* of common.hpp).  Sites: the GEMMs grouped by how much latent / audio error their
    // rounding causes (tests/studies/precision_ladder_cpu.py) and by what they cost.
    enum Site { SITE_DIT_BLOCK = 0,   // QKVG, out-proj, FF1 (SwiGLU), FF2 of the 12 DiT blocks: 95 % of the DiT's flops and bytes
                SITE_ENCODER = 1,     // style / text encoder blocks + their output projections
                SITE_CROSS_KV = 2,    // cross-attention K / V projections of the condition cache
                SITE_COND = 3,        // time / AdaLN modulation chain, latent in-projection, conv pos-embed, velocity head, style in-proj
                SITE_CODEC_FFN = 4,   // codec block FFNs (fused kernels and the wide-stage GEMM pairs)
                SITE_CODEC_CONV = 5,  // codec stem / resampling (ConvTranspose, strided conv) / encoder head GEMMs
                SITE_CONVPOS = 6,     // the grouped conv k = 31 pos-embed of the DiT input embedding (split out of SITE_COND: 1.2 % of a batch's time)
                SITE_ATTN = 7,        // attention operand images (q, k, V^T, sigmoid(gate), P) of the DiT blocks and the encoders
                SITE_COUNT = 8 };
    // preset: 3 = split-bf16 everywhere (fp32-class), 1 = single-pass bf16 everywhere, 2 = "f16 mixed": single-pass fp16 on
    // the block / encoder / cross-KV / codec-FFN GEMMs, split-bf16 on SITE_COND and SITE_CODEC_CONV
    void set_precision(int preset) {
        preset_ = preset == PREC_BF16 ? PREC_BF16 : preset == PREC_F16 ? PREC_F16 : PREC_BF16X3;
        for (int i = 0; i < SITE_COUNT; ++i) prec_[i] = preset_;
        if (preset_ == PREC_F16) prec_[SITE_COND] = prec_[SITE_CODEC_CONV] = prec_[SITE_CONVPOS] = PREC_BF16X3;
    }
    int set_site_precision(int site, int prec) {
        // PREC_F16X2 exists for the codec decoder's ConvTranspose products only (the stages x2_mink_ <= K <= x2_maxk_; the others,
        // the stem and the encoder's strided convs run split-bf16 under it)
        if (site < 0 || site >= SITE_COUNT || prec < 1 || prec > (site == SITE_CODEC_CONV ? PREC_F16X2 : 3))
            return fail("set_site_precision: bad site / precision");
        prec_[site] = prec;
        return 0;
    }
    // Tuning mode.  TUNE_LATENCY (default): one batch at a time should finish as early as possible — split-K on the small-M
    // projections, deep DMA rings, text encoder on the side stream.  TUNE_THROUGHPUT: several independent batches are in flight
    // on the caller's streams (SmallTTS.synthesize_batches, bench.py) — kernels should cost the fewest CU-microseconds and hold
    // the least LDS so that other streams' kernels fit beside them: no split-K, no side stream, persistent codec kernels on three quarters of the CUs (deep rings in both modes since round 3).
    enum { TUNE_LATENCY = 0, TUNE_THROUGHPUT = 1 };
    void set_tuning(int mode);
    int tuning() const { return tuning_; }
    void set_fused_ffn(bool on) { fused_ffn_ = on; }
    void set_attn_img(bool on) { attn_img_ = on; }
    void set_ln_fold(bool on) { ln_fold_ = on; }   // test hook (smtts_test_set_ln_fold): LN-fold on / off, see ln_fold_
    bool ln_fold() const { return ln_fold_; }
    bool attn_img() const { return attn_img_; }
    int site_precision(int site) const { return site >= 0 && site < SITE_COUNT ? prec_[site] : 0; }
    void set_dual_stream(bool on) { dual_stream_ = on; }
    int precision() const { return preset_; }

    // ---- operators (device pointers, async on `st`) ------------------------------------------
    size_t cond_ws_bytes(int B, int R, int P) const;
    int cond_encode(hipStream_t st, const float* ref, const int64_t* ref_len, const int64_t* ids,
                    const uint8_t* ph_mask, int B, int R, int P, float* k_ref, float* v_ref, uint8_t* ref_mask,
                    float* k_text, float* v_text, void* ws, size_t ws_bytes, float* ref_seq_out, float* mem_out);

    size_t denoise_ws_bytes(int B, int N, int R, int P, int rows) const;
    int denoise_step(hipStream_t st, const float* x_t, const uint8_t* mask, const float* t, const float* k_ref,
                     const float* v_ref, const uint8_t* ref_mask, const float* k_text, const float* v_text,
                     const uint8_t* ph_mask, const float* rope, int B, int N, int R, int P, float* velocity,
                     void* ws, size_t ws_bytes);

    // mode 0: DMD re-noising loop (infer/onnx.py:98-125); mode 1: teacher ODE (build-defined).
    // cfg != 0: caches/masks hold 3B rows [cond; no-text; no-speaker], x has B rows.
    // noise: mode 0 -> (n_steps, B, N, 64); mode 1 -> (B, N, 64); null -> Philox(seed).
    size_t sample_ws_bytes(int B, int N, int R, int P, int n_steps, int cfg) const;
    int sample(hipStream_t st, int mode, int n_steps, int cfg, float s_text, float s_spk, const uint8_t* mask,
               const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
               const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P, const float* noise,
               uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes) {
        return sample_align(st, mode, n_steps, cfg, s_text, s_spk, mask, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask, B, N, R, P, noise,
                            seed, x_out, steps_out, ws, ws_bytes, nullptr, 0u, 0u, nullptr);
    }
    // sample() plus the text-attention tap (align.hip): text_mass f32 (B, N, P), DEVICE, caller-owned, ends as the mean over the selected
    // (step, layer, head) triples of each frame's softmax probability on each text key.  sel_steps: HOST array of n_steps flags (null: the
    // last step only); sel_layers / sel_heads: bit masks (bit l / h).  text_mass == null: the tap is off and this is sample() — not one
    // launch more, the latents bit for bit the same either way.
    int sample_align(hipStream_t st, int mode, int n_steps, int cfg, float s_text, float s_spk, const uint8_t* mask,
                     const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
                     const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P, const float* noise,
                     uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes, const uint8_t* sel_steps,
                     unsigned sel_layers, unsigned sel_heads, float* text_mass) {
        return sample_pinned(st, mode, n_steps, cfg, s_text, s_spk, mask, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask, B, N, R, P, noise,
                             seed, x_out, steps_out, ws, ws_bytes, sel_steps, sel_layers, sel_heads, text_mass, nullptr, nullptr, 0);
    }
    // sample_align() that keeps pinned frames (mode 0, cfg == 0; the definition: include/smalltts_hip.h).  x_pin f32 (B, N, 64), pin bool
    // (B, N), both DEVICE; K = pin && mask.  The loop runs steps [start_step, n_steps) from x = x_pin (start_step == 0: K ? x_pin : 0) and
    // writes K ? x_pin : (a x_t - s v) after every step (kernels.hip: pin_renoise / pin_update instead of axpby, no launch more).
    // x_pin == pin == null and start_step == 0: sample_align(), the same kernels.
    int sample_pinned(hipStream_t st, int mode, int n_steps, int cfg, float s_text, float s_spk, const uint8_t* mask,
                      const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
                      const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P, const float* noise,
                      uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes, const uint8_t* sel_steps,
                      unsigned sel_layers, unsigned sel_heads, float* text_mass, const float* x_pin, const uint8_t* pin, int start_step);

    size_t decode_ws_bytes(int B, int T) const;
    int codec_decode(hipStream_t st, const float* latents, int B, int T, float* audio, void* ws, size_t ws_bytes);
    // Streamed decode (include/smalltts_hip.h smtts_codec_decode_stream): T latent frames of B streams whose causal state
    // (the last 8 frames of every image a look-back kernel reads: DecodeStateLayout) lives in slot slots[b] of the caller's pool.  The
    // kernels are codec_decode's at the chunk's (B, T); in front of every consumer carry_frames (codec_stream.hip) puts the carried
    // frames where codec_decode has zeros.  The stage chain is never taken (its warm-up tile special-cases the utterance start).
    struct DecodeStateLayout {   // byte offsets of the boundaries' [8][C] fp32 blocks inside a slot, in slot order
        size_t lat = 0;                           // the latent image (C = latent_dim)
        std::vector<std::vector<size_t>> block;   // [stage][block]: the input of every block
        std::vector<size_t> out;                  // [stage < n_ratios]: the output of a stage that feeds a ConvTranspose
        size_t head = 0;                          // the head's input
        size_t bytes = 0;                         // one slot = the slot stride of a pool: the sum, rounded up to 256
        int count = 0;                            // boundaries
    };
    DecodeStateLayout decode_state_layout() const;   // from the codec spec alone: THE layout, for the size query and the driver
    int codec_decode_stream(hipStream_t st, const float* latents, int B, int T, void* pool, int64_t n_slots, const int64_t* slots,
                            float* audio, void* ws, size_t ws_bytes);
    size_t encode_ws_bytes(int B, int S) const;
    int codec_encode(hipStream_t st, const float* audio, int B, int S, float* latents, void* ws, size_t ws_bytes);

    // The latent phoneme recogniser (asr.hip; include/smalltts_hip.h smtts_asr_logprobs): present when the asr.* tensors were loaded
    size_t asr_workspace_bytes(int B, int N);
    int asr_logprobs(hipStream_t st, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes, float* logp);

    // The latent speaker verifier (sv.hip; include/smalltts_hip.h smtts_sv_embed): present when the sv.* tensors were loaded
    size_t sv_workspace_bytes(int B, int N);
    int sv_embed(hipStream_t st, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes, float* emb);

    const CodecSpecC& codec_spec() const { return cspec_; }
    // per-kernel HIP-event timing (bench.py); report = JSON array, valid after the stream is synchronised
    void profile_enable(int mode);  // 0 off, 1 per-kernel, 2 per-kernel prefixed with the pipeline phase
    std::string profile_report();
    // single-kernel hooks for tests (W* are fp32 [N][K] on the device; split here, freed after the call)
    int test_gemm(hipStream_t st, const float* A, int lda, const float* W, const float* bias, int M, int N, int K,
                  int act, int split, int cfg, float* C, int ldc);
    int test_swiglu(hipStream_t st, const float* A, const float* W1, const float* W3, const float* b1, const float* b3,
                    int M, int F, int K, int split, float* out);

    // microbenchmark: time `iters` launches of one GEMM configuration with HIP events (tools/gemm_bench.py)
    int bench_gemm(int M, int N, int K, int epi, int split, int cfg, int iters, int ver, float* avg_us);
    int test_gemm3(hipStream_t st, const float* A, const float* W, const float* bias, int M, int N, int K, int act,
                   int split, int cfg, float* C);
    int test_ln_fold(hipStream_t st, const float* A, const float* Wp, const float* bp, const float* gate, const uint8_t* mask,
                     const float* nscale, const float* shift, const float* W1, const float* W3, const float* b1, const float* b3,
                     int M, int K, int D, int F, float eps, int rms, int prec, int fold, float* x, float* h,
                     float* c_out);
    // one codec stage through the code of codec_decode (part 1) / codec_encode (part 2): include/smalltts_hip.h smtts_test_codec_stage
    int test_codec_stage(hipStream_t st, int part, int stage, int what, const float* x, int B, int T_in, int C_in, float* out,
                         int* T_out, int* C_out);
    // DiT / encoder stages through the code of denoise_step / sample / cond_encode: include/smalltts_hip.h smtts_test_dit_stage
    int test_dit_stage(hipStream_t st, int net, int what, int l0, int l1, int path, int twice, const void* x, const uint8_t* mask, int B,
                       int S, const float* t, const float* mod, int mod_rows, int mod_row0, int mod_rstride, const float* k_ref,
                       const float* v_ref, const uint8_t* ref_mask, int R, const float* k_text, const float* v_text,
                       const uint8_t* ph_mask, int P, const float* rope, float* x_out, float* img_out, float* shift_out, float* out,
                       float* k_out, float* v_out, float* mod_out);

    // every launch of one recogniser (net 0) / verifier (net 1) call, tapped: include/smalltts_hip.h smtts_test_scorer_taps
    size_t test_scorer_tap_bytes(int net, int B, int N, size_t* off, int cap);
    int test_scorer_taps(hipStream_t st, int net, const float* x, const int32_t* n_len, int B, int N, float* out, void* taps,
                         size_t tap_bytes);

    // fp16 range guard: per-site count of values that fp16 producers clamped to +-65504 since the last reset (device counters,
    // common.hpp sat_note) + the static part: codec FFN blocks whose fused kernels' hidden / input bound could not be certified
    // below the fp16 range at finalize() (those kernels do not count at run time: they are VALU-bound, see finalize_codec).
    // Synchronises the device.
    int get_saturations(unsigned* out, int n, bool reset);
    // the same counts as they stand, while other streams go on working: no device-wide wait and no reset (a reset would race the
    // counting of the batches in flight).  What has COMPLETED before the call is counted in full; work in flight may be counted in part.
    int peek_saturations(unsigned* out, int n);
    const std::string& range_report() const { return range_report_; }
    float range_worst() const { return range_worst_; }

    int fail(const std::string& m) { err_ = m; return 1; }
    int fail_hip(hipError_t e, const char* what);

  private:
    void* dalloc(size_t bytes);
    const RawTensor* raw(const std::string& n) const;
    const float* rawp(const std::string& n) const;
    PW pack_rows(const std::vector<std::string>& names, const std::vector<int>* perm = nullptr, int k_pad = 0);
    PW pack_from_f32(const float* src, int N, int K, int k_pad = 0, int n_pad = 0);
    float* concat_vec(const std::vector<std::string>& names, const std::vector<int>& zero_len = {});
    int finalize_dit();
    int finalize_codec(bool decoder);
    int finalize_asr();
    int finalize_sv();
    struct ScorerPack;   // engine_scorers.hip: a tensor to the host, a packed vector to the device, for both finalizers
    // the six refusals the two scorer entries share.  entry: the C name without "smtts_"; net: "asr" / "sv"; part: what the engine
    // lacks; out: the result's name
    int scorer_entry(const char* entry, const char* net, const char* part, const char* out, bool ready, int n_min,
                     size_t (*ws_need)(int, int), const float* x, const int32_t* n_len, int B, int N, const void* ws, size_t ws_bytes,
                     const float* result);
    int build_encoder(EncoderW& e, const std::string& prefix, int dim, int heads, int ff, int layers, float eps);
    int make_rope(int dim, float** cos_out, float** sin_out);
    struct ModWs;
    int modulation(hipStream_t st, const float* t_dev, int rows, const ModWs& m);   // ... and its LN-fold tables where m plans them
    int fold_tables(hipStream_t st, const float* mod, int rows, float* ftab);   // LN-fold tables of `rows` modulation rows (fold_vectors)
    // ---- condition encoders: one call = per encoder in, blocks [0, L), out, kv.  cond_encode and the test hook (test_dit_stage) run
    // the same functions on workspaces planned the same way (EncWs)
    struct EncWs;
    int style_in(hipStream_t st, const EncWs& w, const float* ref, int B, int R);
    int text_in(hipStream_t st, const EncWs& w, const int64_t* ids, int B, int P);
    // blocks [l0, l1): the RMSNorm of block l0 runs as a launch; ends in the image of block l1's RMSNorm (l1 = L: the final norm) in w.y.
    // fold: the norms between block GEMMs live in their epilogues; ks: K slices of the residual projections outside the fold (1: unsplit)
    int enc_blocks(hipStream_t st, const EncoderW& e, const EncWs& w, int l0, int l1, int B, int S, const uint8_t* key_mask, bool fold,
                   int ks);
    int enc_out(hipStream_t st, bool text, const EncWs& w, int M, const uint8_t* key_mask, float* seq);
    int enc_kv(hipStream_t st, bool text, const EncWs& w, const float* seq, int B, int S, float* k, float* v);
    // cross-KV cache of all layers in the attention kernel's operand format (attention_img.hip), built once per operator call
    struct CrossImg { bf16_t *kc = nullptr, *kc_lo = nullptr, *vtc = nullptr, *vtc_lo = nullptr; int Rp = 0, Cp = 0; };
    struct Cond {   // what a DiT evaluation reads of the conditions: filled once per operator call, where pack_cross runs
        const float *k_ref, *v_ref, *k_text, *v_text;
        const uint8_t *ref_mask, *ph_mask;
        int R, P;
        CrossImg img;
    };
    int pack_cross(hipStream_t st, Cond& c, int B, const CrossImg& carved);   // fills c.img (carved: DitWs) — or leaves it empty
    struct ModRow {   // the modulation row of utterance b is row0 + b rstride of mod; ftab: the LN-fold tables of those rows, or null
        const float* mod = nullptr;
        int row0 = 0, rstride = 0;
        const float* ftab = nullptr;
    };
    struct AlignTap {   // the text-attention tap (sample_align); mass == null: off
        float* mass = nullptr;
        unsigned layers = 0, heads = 0;
        int rows = 0;          // batch rows tapped (the conditional rows of a CFG batch)
        float scale = 0.f;     // 1 / selected (step, layer, head) triples
        bool first = true;     // the next tap stores, later ones add
        bool step_on = false;  // the step being evaluated is selected
    };
    struct AuxSet { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
    // The host state of ONE operator call (sample_pinned, denoise_step, test_dit_stage), handed down by reference
    struct Call {
        hipStream_t st;
        const AuxSet* side = nullptr;   // the side set of this caller stream; null: the call does not fork
        bool join_owed = false;         // the side stream's modulation table must be joined before the first AdaLN reads it
        bool ws_zeroed = false;         // the regions of the workspace no kernel writes were zeroed by an earlier evaluation of this call
        AlignTap tap;                   // dit_blocks moves first / step_on
        explicit Call(hipStream_t s) : st(s) {}
        Call(const Call&) = delete;
        hipError_t join() {
            const hipError_t e = join_owed ? hipStreamWaitEvent(st, side->join, 0) : hipSuccess;
            if (e == hipSuccess) join_owed = false;
            return e;
        }
        // an early return between the fork and the first AdaLN must not leave the side stream's writes into this workspace unordered
        // against whatever the caller does next on `st`
        ~Call() { (void)join(); }
    };
    // ---- DiT: one evaluation = embed, blocks [0, 12), head (denoise_core); the modulation table comes from modulation()
    struct CoreWs;
    struct DitWs;
    size_t dit_ws_bytes(int B, int N, int R, int P, int mod_rows, bool fold, int n_steps, int cfg) const;
    struct DitRun {   // what the block stages read besides the residual stream (dit_run)
        const uint8_t* mask = nullptr;
        ModRow row;
        const Cond* cond = nullptr;
        const float *rc = nullptr, *rs = nullptr;   // rope cos / sin [N][64]
        const float* frow = nullptr;   // LN-fold tables of this step's modulation row: non-null = the fold path
        int ks_out = 1, ks_ff2 = 1;    // K slices of the out-proj / FF2 launches outside the fold (1: unsplit GEMM + ln_modulate)
        int B = 0, N = 0;
    };
    int dit_run(hipStream_t st, const CoreWs& w, const uint8_t* mask, const ModRow& row, const Cond& cond, const float* rope, int B, int N,
                bool fold, bool unsplit, DitRun& d);
    int denoise_core(hipStream_t st, const float* x_t, const uint8_t* mask, const ModRow& row, const Cond& cond, const float* rope, int B,
                     int N, float* velocity, const CoreWs& w, Call& call);
    int dit_embed(hipStream_t st, const CoreWs& w, const float* x_t, const uint8_t* mask, int B, int N, bool init_ws);
    // blocks [l0, l1): the AdaLN of block l0 runs as the ln_modulate launch (and seeds the fold's row shift); each block ends in the
    // next block's AdaLN image in w.y — after block 11 the final AdaLN (SITE_COND format)
    int dit_blocks(hipStream_t st, const CoreWs& w, const DitRun& d, int l0, int l1, Call& call);
    int dit_head(hipStream_t st, const CoreWs& w, int M, float* velocity);
    int ensure_qkvg_unpadded();   // packs DitBlockW::qkvg of every block on first use of an A/B attention path
    bool qkvg_unpadded_ready_ = false;   // ... set only after EVERY block packed (a failure half-way unlinks what was built)
    // ---- codec: one call = stem, then per stage the resampling into it (stage > 0) and its blocks, then final norm + head.  The
    // operators and the test hook (test_codec_stage) run the same functions on a workspace planned the same way (codec_plan).
    struct CodecPlan { size_t max_img = 0, max_hid = 0, lat = 1; };   // elements: one image, one FFN hidden, the decoder's latent image
    struct CodecWs;
    CodecPlan codec_plan(bool decoder, int B, long T) const;   // T: decoder latent frames / encoder audio samples of the whole call
    size_t codec_ws_bytes(const CodecPlan& p) const;
    // cy (streamed decode): where these zero pad frames, they carry them instead, on the image the next consumer reads, in front of it
    struct CodecCarry {
        void* pool; long stride, n_slots; const int64_t* slots; const DecodeStateLayout* lay;
        hipError_t run(float* img, int B, int T, int C, size_t off, hipStream_t st) const {
            return launch_carry_frames(img, B, T, C, pool, stride, (long)off, n_slots, slots, st);
        }
    };
    int decode_stem(hipStream_t st, const CodecWs& w, const float* latents, int B, int T, const CodecCarry* cy = nullptr);
    int decode_stage(hipStream_t st, const CodecWs& w, int i, int what, float** x, float** xn, int B, int* Ti, int* C,
                     const CodecCarry* cy = nullptr);
    int decode_head(hipStream_t st, const CodecWs& w, float* x, int B, int Ti, int C, float* audio, const CodecCarry* cy = nullptr);
    int encode_stem(hipStream_t st, const CodecWs& w, const float* audio, int B, int S);
    int encode_stage(hipStream_t st, const CodecWs& w, int i, int what, float** x, float** xn, int B, int* Ti, int* C);
    int encode_head(hipStream_t st, const CodecWs& w, const float* x, int B, int Ti, int C, float* latents);
    int conv_small_m(hipStream_t st, const CodecWs& w, const float* img, long img_rows, int Cin, const RowMap& am, const PW& wt,
                     const float* bias, float* out, const RowMap& om, int M);
    int codec_stage_chain(hipStream_t st, const CodecStageW& sg, float** x, float** xalt, int B, int T, int C);
    int codec_block(hipStream_t st, const CodecBlockW& w, float** x, float** xalt, float* nbuf, bf16_t* n2hi, bf16_t* n2lo,
                    bf16_t* hhi, bf16_t* hlo, int B, int T, int C, size_t n2_elems /* capacity of n2hi (bf16 elements) */,
                    bool carried = false /* the pad frames of *x hold carried frames: a path that reads pads of nbuf normalises them too */);
    int check_shape(const std::string& name, std::initializer_list<long> want);
    void invalidate() { finalized_ = false; dit_ready_ = false; dec_.ready = false; enc_.ready = false; asr_ready_ = false; sv_ready_ = false; }
    void free_packs();

    // the tag a producer of attention operand images is handed in place of the (unused) lo array when the images are fp16
    bf16_t* img_lo(int pa, bf16_t* lo) const { return pa == PREC_F16 ? sm_lo_for(PREC_F16, nullptr, satp(SITE_ATTN)) : lo; }
    int certify_codec_ffn(const std::string& name, CodecBlockW& b, int C, int F);
    unsigned* sat_ = nullptr;                 // [SITE_COUNT] device counters (null if the allocation failed: nothing is counted)
    unsigned* satp(int site) const { return sat_ ? sat_ + site : nullptr; }
    unsigned sat_static_[SITE_COUNT] = {};    // uncertified fused-kernel blocks (set by finalize)
    float* cert_scratch_ = nullptr;           // 2 floats: max hidden bound, max input bound
    std::string range_report_;
    float range_worst_ = 0.f;                 // largest certified bound of the last finalize (diagnostic)

    int device_;
    std::string err_;
    std::map<std::string, RawTensor> raw_;
    std::vector<void*> allocs_;       // raw fp32 tensors (live as long as the engine)
    std::vector<void*> pack_allocs_;  // everything finalize() builds: freed and rebuilt by the next finalize()
    bool packing_ = false;
    int tuning_ = TUNE_LATENCY;
    LaunchTuning tune_;          // what every launcher that reads tuning is handed next to the stream (common.hpp).  set_tuning() moves two fields: the ring
                                 // depth (1 under both tunings since round 3; SMTTS_GEMM_DEEP) and the persistent codec grids' cap: 0 under latency tuning,
    int persist_cus_tp_ = 192;   // this under throughput tuning (SMTTS_PERSIST_CUS; profiles/r03ac_*, r03ad_*)
    bool dual_stream_latency_ = true;  // the dual-stream setting that TUNE_LATENCY restores
    int preset_ = kDefaultPrecision;   // set_precision(kDefaultPrecision) in the constructor fills prec_
    int prec_[SITE_COUNT] = {3, 3, 3, 3, 3, 3, 3, 3};
    bool fused_ffn_ = true;  // test hook: smtts_test_set_fused_ffn
    bool small_m_splitk_ = true;   // SMTTS_SMALLM_SPLITK=0: A/B switch for the K-sliced small-M products of the codec
    int chain_min_run_ = 16;   // ... and decodes of at least this many tiles per wave of the chain's grid (codec_stage_chain)
    int chain_min_blocks_ = 2; // ... for stages of at least this many blocks (a single block gains nothing from the chain's contiguous walk; SMTTS_CHAIN_MIN=1: debugging)
    bool stage_chain_ = true; // codec stages with C = 32: all blocks of the stage in ONE launch (SMTTS_STAGE_CHAIN=0: one launch per block)
    bool block_wave_ = true;  // codec stages with C = 32 / 64: mixer + FFN in one kernel (SMTTS_BLOCK_WAVE=0: mixer_fused + codec_ffn_wave)
    bool mixer_wide_ = true;   // codec blocks of the wide stages: mixer + FFN norm in one pass (SMTTS_MIXER_WIDE=0: rmsnorm + dwconv_resid_rms)
    int x2_mink_ = 512, x2_maxk_ = 1024;   // PREC_F16X2 on SITE_CODEC_CONV: the ConvTranspose stages with K in this range (SMTTS_X2_MINK / _MAXK)
    int up_g3_mink_ = 2048;  // codec ConvTranspose-as-GEMM: gemm3 on a converted copy of the image from this K up (SMTTS_UP_G3_MINK; below: fp32-A kernel)
    int ksplit_enc_ = 4;  // split-K of the encoders' residual projections (1 = fused-epilogue GEMM + separate RMSNorm)
    int ksplit_out_ = 2, ksplit_ff2_ = 2;  // (<= kSplitK) split-K factors of the two N = 960 DiT projections in latency tuning (1 = fused epilogue).  Round 5
                                           // (profiles/r05h_splitk_table.txt, three interleaved repeats on one box): 2 slices 11.75-11.79 ms per batch one at a
                                           // time, 3 slices (rounds 1-4: 450 workgroups = one round at 2 per CU) 11.86-11.87, unsplit + ln_modulate 11.90-11.98 —
                                           // a launch of these 600-row products is ~8 us of fixed cost whatever its k-loop (5 k-tiles at 3 slices), so the third
                                           // slice only adds a partial slab (a third of the fp32 slab traffic of the reduce kernel)
    bool dual_stream_ = true;  // cond_encode: text encoder on a side stream (SMTTS_SINGLE_STREAM=1 turns it off)
    std::map<hipStream_t, AuxSet> aux_sets_;      // side stream + fork / join events per caller stream: complete entries only
    const AuxSet* side_set(hipStream_t st);       // ... looked up, created on a stream's first fork; null with err_ set on failure
    int num_cus_ = 256;
    bool convpos_by_group_ = true;  // grouped conv pos-embed as one product per group over the batch's rows (false: per (utterance, group))
    bool attn_img_ = true;   // attention on producer-written operand images (attention_img.hip: DMA + MFMA only); false (SMTTS_ATTN_IMG=0, test hook) = fp32 projection + qk_prep + the fp32 VALU reference kernel (attention.hip)
    // LN-fold (round 6; gemm.hpp LnFoldIn): inside the fused sampler (one modulation row per step for the whole batch) the AdaLN in front
    // of the QKVG / FF1 products is folded into the producing out-proj / FF2 epilogue (operand image + row partials) and the consuming
    // epilogue (mean / rstd correction): no split-K partials + reduce launches in latency tuning — 5 launches per DiT block (and per
    // encoder block: RMSNorm variant, no tables) instead of 7 (SMTTS_LN_FOLD=0 / smtts_test_set_ln_fold restore the norm launches)
    bool ln_fold_ = true;
    // ... under THROUGHPUT tuning too.  Off: with batches in flight the DiT fold's per-call table kernel (fold_vectors: every block weight
    // read once more, 205 MB = 80 us of the whole chip) costs more than the ln_modulate launches it replaces, and the encoders' unsplit
    // 16-workgroup products no less than their split-K 4 + reduce pairs — measured (profiles/r06i_ab_fold.txt, three interleaved repeats):
    // in flight 8.19 (off) / 8.22 (encoders only) / 8.26 (all) ms per batch, one at a time 11.77 -> 11.62 (SMTTS_LN_FOLD_TP=1: A/B)
    bool ln_fold_tp_ = false;
    bool ln_fold_now() const { return ln_fold_ && (tuning_ == TUNE_LATENCY || ln_fold_tp_); }
    bool attn_epi_ = true;   // ... written by the QKVG GEMM's own epilogue (gemm3 EpiQKV); false (SMTTS_ATTN_EPI=0): fp32 projection + qkv_pack kernel
    // THE fold predicates: every buffer and launch of the LN-fold (tables, row partials, row shifts) follows them.  The QKV consumer is
    // the attention epilogue (EpiQKV), so no epilogue attention, no fold
    bool fold_epi_on() const { return ln_fold_now() && attn_img_ && attn_epi_; }
    bool dit_fold_on(long rows) const;   // the fused sampler's DiT blocks, rows = batch rows (engine.hip)
    Profiler prof_;
    bool prof_on_ = false;
    bool finalized_ = false;

    // DiT packs
    bool dit_ready_ = false;
    PW time0_, time2_, emb0_, emb2_, modall_, inproj_, conv1_, conv2_, velocity_, phproj_, kvref_, kvtext_, style_in_,
        style_out_;
    float *modall_b_ = nullptr, *kvref_b_ = nullptr, *kvtext_b_ = nullptr, *knc_ = nullptr;
    std::vector<DitBlockW> blocks_;
    EncoderW style_, text_;
    float style_scale_ = 1.f;
    float *rope_dit_cos_ = nullptr, *rope_dit_sin_ = nullptr;  // [MAXPOS][64]

    CodecSpecC cspec_;
    CodecHalfW dec_, enc_;

    bool asr_ready_ = false;
    AsrW asr_{};

    bool sv_ready_ = false;
    SvW sv_{};
};

void alpha_sigma_host(float t, float& a, float& s);

static constexpr int kMaxPos = 4096;   // reference rope tables (dit.py:139, style.py:140)
static constexpr int kHidden = 960, kHeads = 8, kDh = 120, kBlocks = 12, kFF = 2400, kLatent = 64;
static constexpr int kSplitK = 4;   // K slices of the DiT out-proj / FF2 GEMMs
static constexpr int kFFp = 2432;  // FF hidden row stride: 2400 padded to a multiple of 64 (zero tail) for the DMA GEMM
static constexpr int kModPerBlock = 6 * kHidden;
static constexpr long kModLd = (long)kBlocks * kModPerBlock + 2 * kHidden;  // 71040
static constexpr int kConvK = 31, kConvG = 16, kConvCpg = 60, kConvPad = 15, kConvGs = 64;
static constexpr int kCodecPad = 8;
static constexpr long kFoldPerBlock = 4L * kHeads * 128 + 2L * kFF;   // LN-fold table columns of one block: padded QKVG rows | interleaved [w1 | w3] rows
static constexpr long kFoldNF = kBlocks * kFoldPerBlock;              // 106752
static constexpr long kFoldMaxRows = 1024;                            // LN-fold of the DiT blocks up to this many rows (above: unsplit GEMM + ln_modulate, as before)
static constexpr int kLnGroups = kHidden / 32;                        // row partials per residual row
