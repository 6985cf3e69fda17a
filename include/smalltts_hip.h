/* smalltts_hip.h — C ABI of libsmalltts_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the four opaque onnxruntime graphs the reference drives
 * (SURVEY.md §8b).  Each entry point cites the reference interface it replaces
 * (paths relative to the reference repository root):
 *
 *   smtts_cond_encode   <- condition_encoder.onnx   src/smalltts/infer/onnx.py:91-96,
 *                                                   src/server/src/pipeline.rs:122-141  (= DiTModel.encode_conditions,
 *                                                   src/smalltts/models/backbone/model.py:88-95)
 *   smtts_denoise_step  <- denoiser.onnx            src/smalltts/infer/onnx.py:107-124,
 *                                                   src/server/src/pipeline.rs:143-166  (= DiTModel.denoise_step, model.py:97-100)
 *   smtts_sample        <- the host-side sampler loop src/smalltts/infer/onnx.py:98-125, pipeline.rs:84-93
 *                          (mode 1: teacher ODE + CFG, built from src/scripts/train/dmd2/distill.py:60-134)
 *   smtts_codec_decode  <- codec/decoder.onnx       src/smalltts/codec/onnx.py:34-53, infer/onnx.py:127-128
 *   smtts_codec_encode  <- codec/encoder.onnx       src/smalltts/codec/onnx.py:56-75
 *
 * Conventions: plain C types only; every tensor argument is a DEVICE pointer on the handle's GPU
 * (e.g. torch tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream);
 * all work is enqueued asynchronously on `stream`.  The caller owns inputs, outputs and workspace
 * (query the size first); the library owns weights only.  Return 0 = ok, non-zero = error with the
 * message available from smtts_last_error().
 * A workspace (`ws`) must be 256-BYTE ALIGNED: the library carves it at 256-byte offsets from its base and keeps an operand-format
 * tag in the low bits of the carved addresses.  hipMalloc and torch's allocator return such addresses; a sub-allocation of the
 * caller's own arena must be placed on a 256-byte boundary.  Every entry that takes `ws` refuses a misaligned one (non-zero,
 * "workspace must be 256-byte aligned") next to its "workspace too small" check, before anything is enqueued.
 *
 * Threading / streams (the same rules as smalltts_amd/csrc/engine.hpp:4-8): a handle is NOT thread-safe — one handle per GPU,
 * driven by ONE host thread (the reference also has one Session per pipeline behind a mutex, src/server/src/main.rs:24,138).
 * That thread MAY keep several operator calls in flight on DIFFERENT streams, provided that
 *   (1) every call in flight has its own workspace and its own output buffers (all per-call scratch lives in the workspace;
 *       weights are read-only after smtts_finalize);
 *   (2) smtts_set_tuning(h, 1) ("throughput") was selected first: kernels that cost the fewest CU-microseconds, no side streams
 *       (the side stream of smtts_cond_encode / smtts_sample belongs to the caller's stream — one per caller stream — so calls in
 *       flight would not share it, but six streams for three batches run 20 % slower than three: profiles/r06j_ab_dual_tp.txt);
 *   (3) per-kernel profiling (smtts_profile_enable) is off: it assumes one call at a time.
 * Calls on one stream are ordered like any other work on that stream; results do not depend on what runs on the other streams
 * (tests/test_api_gpu.py::test_results_repeat_bit_for_bit_next_to_other_streams).
 * bool tensors are 1 byte per element (numpy/torch bool).
 */
#ifndef SMALLTTS_HIP_H
#define SMALLTTS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smtts_engine* smtts_handle;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int smtts_create(int device_id, smtts_handle* out);
int smtts_destroy(smtts_handle h);
const char* smtts_last_error(smtts_handle h); /* h may be NULL: last creation error */
const char* smtts_version(void);
/* bumped on every signature / default change: 11 = smtts_sample_align, smtts_align_path, smtts_test_attn_text_mass (+ smtts_sample_pinned, then smtts_take_scores and smtts_take_select, then the streamed decode entries, then smtts_deliver, then smtts_join_stream and smtts_peek_saturations, then the smtts_watermark entries, then smtts_retime, then smtts_pitch, additive: no existing signature or default changed, no bump); 10 = smtts_endpoints, smtts_stitch_seg; 9 = smtts_voice_expand, smtts_randn_rows, smtts_stitch; 8 = smtts_test_dit_stage; 7 = smtts_test_codec_stage; 6 = smtts_test_ln_fold; 5 = round 6 (smtts_test_set_ln_fold; one side stream per caller stream); 4 = round 4 (workspace queries take R and P, new handles default to preset 2,
 * smtts_get_saturations) */
#define SMTTS_ABI_VERSION 11
int smtts_abi_version(void);

/* ---- weights (replaces the ONNX initialisers; names/shapes = DiTModel.state_dict(),
 *      src/scripts/test_checkpoint.py:44-73, plus codec.* names of smalltts_amd/weights.py) ---- */
int smtts_set_tensor(smtts_handle h, const char* name, const float* data, const int64_t* shape, int ndim,
                     int data_on_device);
int smtts_synth_tensor(smtts_handle h, const char* name, const int64_t* shape, int ndim, uint64_t key, float mean,
                       float half_range);
int smtts_get_tensor(smtts_handle h, const char* name, float* host_out, int64_t numel);
/* codec hyper-parameters (decoder order); must precede smtts_finalize when codec tensors are present */
int smtts_set_codec_spec(smtts_handle h, int latent_dim, int n_filters, int kernel, int ffn_mult, float eps,
                         const int* ratios, int n_ratios, const int* depths /* n_ratios + 1 */);
int smtts_finalize(smtts_handle h);
/* GEMM operand precision preset (fp32 accumulation, fp32 residual stream / norms / softmax / sampler state in all of them):
 *   2 = "f16 mixed" — THE DEFAULT of a new handle (smtts_default_precision() == 2; the Python host side sets the same):
 *       ONE fp16 MFMA per product on the DiT-block / encoder / cross-KV / codec-FFN GEMMs (>= 95 % of the flops and
 *       weight bytes), split-bf16 on the conditioning chain, latent in / out projections and codec resampling convs
 *       (measured: latent rel-L2 ~1.5e-4 vs the fp32 oracle, inside the 1e-3 contract)
 *   3 = split-bf16 everywhere: x = hi + lo, three bf16 MFMAs per product (fp32-class results, ~1.4x the time)
 *   1 = single-pass bf16 everywhere (latent rel-L2 ~4e-3: outside the 1e-3 contract, kept for A/B) */
int smtts_set_precision(smtts_handle h, int preset);
int smtts_get_precision(smtts_handle h);   /* the preset in force (1 / 2 / 3) */
int smtts_default_precision(void);         /* host-only: the preset smtts_create starts with */
/* one GEMM site group at a time: site 0 DiT blocks, 1 encoders, 2 cross-KV, 3 conditioning / in / out projections,
 * 4 codec FFNs, 5 codec stem / resampling convs, 6 conv pos-embed, 7 attention operands (q, k, v, gate, probabilities);
 * prec 1 bf16, 2 fp16, 3 split-bf16 (call after smtts_set_precision); site 5 (codec resampling convs) also takes
 * 4 = "fp16 x 2": fp16 activations against fp16 hi + lo weights, two passes instead of split-bf16's three, on the decoder's
 * ConvTranspose stages with 512 <= K <= 1024 (the other stages stay split-bf16) */
int smtts_set_site_precision(smtts_handle h, int site, int prec);
/* fp16 range guard.  fp16 operands saturate at +-65504 instead of overflowing to inf, which is silent; every producer of an
 * fp16 operand therefore counts the values it had to clamp into a per-site device counter (sites as above).  counts[i] = clamps
 * of site i since the last reset; for site 4 additionally the number of fused codec FFN blocks whose hidden / input range could
 * not be certified from the weights at smtts_finalize (those kernels carry no run-time check; smtts_range_report names them).
 * Non-zero = the results of that site are clipped: re-run with smtts_set_site_precision(site, 3) (split-bf16 has fp32 range) —
 * smalltts_amd/api.py does that automatically.  Synchronises the device.  Real checkpoints enter through
 * src/scripts/train/dmd2/distill.py:468-479; the SwiGLU hidden (models/backbone/dit.py:176-186) is the likeliest site. */
int smtts_get_saturations(smtts_handle h, uint32_t* counts, int n_sites, int reset);
/* the same counts as they stand, for callers that keep batches in flight: no device-wide wait and no reset (a reset would
 * race the counting of the work in flight).  Whatever had COMPLETED before the call is counted in full; work still running may be
 * counted in part.  A site that clamped keeps its count until the next smtts_get_saturations(reset = 1). */
int smtts_peek_saturations(smtts_handle h, uint32_t* counts, int n_sites);
const char* smtts_range_report(smtts_handle h);      /* "" when every fused FFN block was certified */
float smtts_range_worst_bound(smtts_handle h);       /* largest certified bound of the last finalize (fp16 max: 65504) */
int smtts_has_part(smtts_handle h, int part); /* 0 dit, 1 codec decoder, 2 codec encoder, 3 latent phoneme recogniser (asr.* tensors), 4 latent speaker verifier (sv.* tensors) */

/* ---- condition encoder ---------------------------------------------------------------------- */
size_t smtts_cond_workspace_bytes(smtts_handle h, int B, int R, int P);
/* ref f32 (B,R,64); ref_len i64 (B); phonemes i64 (B,P); ph_mask bool (B,P)
 * -> k_ref,v_ref f32 (12,B,8,R,120); ref_mask bool (B,R); k_text,v_text f32 (12,B,8,P,120).
 * ref_seq_out (B,R,960) / mem_out (B,P,960) are optional debug taps (NULL to skip). */
int smtts_cond_encode(smtts_handle h, void* stream, const float* ref, const int64_t* ref_len, const int64_t* phonemes,
                      const uint8_t* ph_mask, int B, int R, int P, float* k_ref, float* v_ref, uint8_t* ref_mask,
                      float* k_text, float* v_text, void* ws, size_t ws_bytes, float* ref_seq_out, float* mem_out);

/* ---- denoiser --------------------------------------------------------------------------------- */
size_t smtts_denoise_workspace_bytes(smtts_handle h, int B, int N, int R, int P);
/* x_t f32 (B,N,64); mask bool (B,N); t f32 (B); caches as above; rope f32 (1,N,64) angles or NULL
 * -> velocity f32 (B,N,64) */
int smtts_denoise_step(smtts_handle h, void* stream, const float* x_t, const uint8_t* mask, const float* t,
                       const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
                       const float* v_text, const uint8_t* ph_mask, const float* rope, int B, int N, int R, int P,
                       float* velocity, void* ws, size_t ws_bytes);

/* ---- sampler ---------------------------------------------------------------------------------- */
size_t smtts_sample_workspace_bytes(smtts_handle h, int B, int N, int R, int P, int n_steps, int cfg);
/* mode 0: x=0; for t in linspace(1,0,n): x_t = a x + s eps_i; v = denoise; x = a x_t - s v  (DMD student)
 * mode 1: deterministic ODE from x_1 = s(1) eps (teacher), see DESIGN.md
 * cfg != 0: mask/caches/cond masks carry 3B rows [cond; text dropped; speaker dropped]; x has B rows;
 *           v = vc + s_text (vc - vt) + s_spk (vc - vs).
 * noise: mode 0 (n_steps,B,N,64), mode 1 (B,N,64); NULL -> on-device Philox4x32-10 with `seed`.
 * x_out (B,N,64); steps_out optional (n_steps,B,N,64) x-hat after every step. */
int smtts_sample(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                 const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                 const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                 const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes);

/* ---- word timings (DESIGN.md 'Word timings') ---------------------------------------------------
 * smtts_sample with the text-attention tap: for the selected (step, layer) pairs a kernel behind the joint attention re-reads its
 * operand images and masks, recomputes each valid frame's softmax over ALL valid keys [self | reference | text] in fp32 and adds the
 * probabilities of the text keys of the selected heads into text_mass f32 (B,N,P), DEVICE, caller-owned (cfg: the B conditional rows).
 * The first tap stores, later ones add; on return (stream order) text_mass is the MEAN over the selected (step, layer, head) triples:
 * every frame's row sums to at most 1.  Exactly 0 for frames outside `mask`, for text columns outside ph_mask and for rows without
 * a valid key.  No atomics, a fixed reduction order: two calls return the same bits, whatever runs on other streams.
 *   tap_steps: HOST array of n_steps flags, NULL = the last step only (t = 0); tap_layers: bit l = DiT block l (12); tap_heads: bit h
 *   = head h (8); a selection without a step, layer or head is an error.  Which layers / heads align best on trained weights has not
 *   been measured: the selection is the caller's.
 * text_mass == NULL: exactly smtts_sample (no extra launch).  x_out is bit-identical with and without the tap.  If the attention
 * operand-image path is switched off (smtts_test_set_attention_mfma(h, 0)) a tap request is an error, never a buffer of zeros. */
int smtts_sample_align(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                       const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                       const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                       const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes,
                       const uint8_t* tap_steps, uint32_t tap_layers, uint32_t tap_heads, float* text_mass);
/* ---- pinned sampling (DESIGN.md 'Re-speaking part of an utterance') ----------------------------------
 * smtts_sample_align that keeps pinned frames: the DMD sampler re-noises its current estimate at every step, so a frame whose
 * estimate is overwritten with a known latent after every step stays exactly that latent, and every other frame is denoised with
 * the known frames in view, at the right noise level, through the joint self-attention (RePaint-style conditioning for an x0
 * sampler; no training).  x_pin f32 (B,N,64) and pin bool (B,N), both DEVICE.  With K[b][n] = pin[b][n] && mask[b][n] (pin == NULL:
 * all false):
 *     x = (start_step == 0) ? (K ? x_pin : 0) : x_pin
 *     for i in start_step .. n_steps-1:
 *         x_t = al[i] * x + sg[i] * eps_i        eps_i: noise[i], or Philox(seed, stream i): always stream i, whatever start_step is
 *         v   = denoise(x_t, t_i)                unchanged
 *         x   = K ? x_pin : (al[i] * x_t - sg[i] * v)
 *         steps_out[i] = x                       slots below start_step are not written
 *     x_out = x
 * Mode 0 (DMD) and cfg == 0 only; 0 <= start_step < n_steps; start_step > 0 needs x_pin; pin != NULL needs x_pin; x_pin and noise
 * 16-byte aligned (the workspace 256-byte, as everywhere); anything else returns 1 with a message before anything is enqueued.  Workspace:
 * smtts_sample_workspace_bytes.  The tap arguments work as in smtts_sample_align; a flagged step below start_step is not run and does
 * not count in the tap's mean, and a selection with no step left is an error.  The select rides in the two element-wise kernels of a
 * step (16-byte lanes, sixteen of them share a frame's pin byte): not one launch more than smtts_sample.  With x_pin given, pin all
 * false and start_step == 0, x_out and steps_out equal smtts_sample's bit for bit; with x_pin == NULL, pin == NULL and start_step
 * == 0 this IS smtts_sample_align, the same kernels.
 * Only this mechanism is verified.  It is UNVALIDATED on trained weights: every weight this project has run is seeded noise, and
 * nobody has measured how well a 4-step distilled student inpaints: whether the regenerated frames join the kept ones audibly well
 * is for whoever holds a trained checkpoint to measure. */
int smtts_sample_pinned(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                        const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                        const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                        const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes,
                        const uint8_t* tap_steps, uint32_t tap_layers, uint32_t tap_heads, float* text_mass, const float* x_pin,
                        const uint8_t* pin, int start_step);
/* monotone alignment of mass f32 (B,N,P), one workgroup per row, on `stream`. n_len, p0, p1: int32 (B) DEVICE arrays (clamped to the
 * shape): frames [0, n_len[b]), tokens [p0[b], p1[b]) — p0 skips a prepended transcription.  cost c[n][p] = 1 - mass[b][n][p];
 * D[n][p] = c[n][p] + min(D[n-1][p-1], D[n-1][p], D[n][p-1]), ties prefer the diagonal, then (n-1,p), then (n,p-1); the path runs from
 * (0, p0) to (n_len - 1, p1 - 1).  -> spans int32 (B,P,2) = (first, last) frame of every token on the path, (-1,-1) for tokens outside
 * the range and for empty rows; score f32 (B) = the path cost (0 for empty rows).  One resolution step = one codec frame (hop samples).
 * Every step is a single fp32 operation in a fixed order: numpy float32 reproduces spans and score bit for bit.  1 <= N <= 225 and
 * 1 <= P <= 198 (the API's range), anything else is an error. */
int smtts_align_path(smtts_handle h, void* stream, const float* mass, int B, int N, int P, const int32_t* n_len, const int32_t* p0,
                     const int32_t* p1, int32_t* spans, float* score);

/* ---- takes (DESIGN.md '8d. Takes'): sample every row K times, keep the best-aligned take on the device ----------------------------
 * smtts_take_scores, behind smtts_align_path on `stream`, one workgroup per row: mass f32 (B,N,P) (the tap), spans i32 (B,P,2) and
 * path_score f32 (B) (smtts_align_path's outputs), n_len / p0 / p1 i32 (B), all DEVICE; n, p0, p1 are clamped exactly as
 * smtts_align_path clamps them (n into [0, N], p0 and p1 into [0, P]), Pw = p1 - p0.  For a row with n > 0 and Pw > 0, with
 * (first_p, last_p) = spans[b][p]: a span with first_p < 0 or last_p < first_p is EMPTY (length 0, and its token counts as skipped);
 * of any other span both ends are clamped into [0, n - 1] before anything is indexed, and its length is last_p - first_p + 1 of the
 * clamped ends.  Four integer features:
 *     cells   = sum over p in [p0, p1) of the span lengths
 *     skipped = number of p in [p0, p1) without a frame f in [first_p, last_p] with mass[b][f][p] >= tau_tok   (the span's peak stays
 *               below the threshold; an empty span is skipped)
 *     longest = max over p in [p0, p1) of the span lengths
 *     idle    = number of frames f < n without a token p in [p0, p1) with mass[b][f][p] >= tau_frm
 * Every comparison is made on one fp32 value: a value equal to the threshold attends, a NaN never does (a span of NaNs is skipped, a
 * frame of NaNs is idle), and no reduction order can change a feature.  Then, as single correctly rounded fp32 operations in this
 * order (no fma):
 *     c0 = path_score[b] / (float)cells      c1 = (float)skipped / (float)Pw      c2 = (float)longest / (float)n
 *     c3 = (float)idle / (float)n            total = ((w0 * c0 + w1 * c1) + w2 * c2) + w3 * c3
 * Rows with n == 0 or Pw <= 0: features 0, total = +inf.  -> feat i32 (B,4) = (cells, skipped, longest, idle), total f32 (B); lower is
 * better.  numpy float32 reproduces both bit for bit (the payload of a NaN total, e.g. from cells == 0, is not specified).  No index
 * leaves the row whatever the buffers hold.  1 <= N <= 225, 1 <= P <= 198, 1 <= B <= 65536; the weights >= 0 and the thresholds not NaN.
 *
 * smtts_take_select: rows are piece-major, row = g * K + k, 1 <= K <= 16, B = G * K, 1 <= G <= 65535.  Key of a take: s' = isnan(total) ?
 * +inf : total.  The winner of group g is the lowest k with the smallest s' (strict < walking k upward: ties and groups that are +inf
 * throughout give k = 0).  Row g * K + winner of x f32 (B,N,64), n_len i32 (B) and, where given, spans i32 (B,P,2) and mass f32 (B,N,P)
 * is copied to row g of x_win (G,N,64), n_win (G), spans_win (G,P,2), mass_win (G,N,P), bit for bit (16-byte lanes where a row's byte
 * count and both base addresses allow, 4-byte elements otherwise: no alignment is required); winner i32 (G) = the k.  spans / spans_win
 * and mass / mass_win are each given or NULL together; a NULL pair is skipped.  Inputs and outputs must not overlap.
 *
 * Both: an argument error (NULL handle or required pointer, B / G / K / N / P out of range, half an optional pair, a negative or NaN
 * weight, a NaN threshold) returns 1 with a message naming the entry before anything is enqueued.  One launch each, no atomics, no
 * synchronisation: two calls return the same bits.
 * Only this mechanism is verified.  Whether the total ranks takes the way a listener would is UNVALIDATED on trained weights: every
 * weight this project has run is seeded noise, the weights and thresholds the Python side passes by default (api.Takes) are design
 * choices and not measurements, and the tap's layer / head selection they rest on is unvalidated in the same way. */
int smtts_take_scores(smtts_handle h, void* stream, const float* mass, const int32_t* spans, const float* path_score, const int32_t* n_len,
                      const int32_t* p0, const int32_t* p1, int B, int N, int P, float tau_tok, float tau_frm, float w0, float w1, float w2,
                      float w3, int32_t* feat, float* total);
int smtts_take_select(smtts_handle h, void* stream, const float* total, int G, int K, int N, int P, const float* x, const int32_t* n_len,
                      const int32_t* spans /* or NULL */, const float* mass /* or NULL */, float* x_win, int32_t* n_win,
                      int32_t* spans_win, float* mass_win, int32_t* winner);

/* ---- repair (DESIGN.md '8e. Repair'): re-speak only the badly aligned words of a take, on the device -----------------------------
 * smtts_repair_plan, behind smtts_align_path (and smtts_take_select) on `stream`, one workgroup per row, writes the pin mask that
 * smtts_sample_pinned takes: mass f32 (B,N,P) (the tap), spans i32 (B,P,2) (smtts_align_path's output), n_len / p0 / p1 i32 (B), keep u8
 * (B,N) or NULL, all DEVICE; n, p0, p1 are clamped exactly as smtts_take_scores clamps them (n into [0, N], p0 and p1 into [0, P]).  For
 * a token p in [p0, p1) with (first, last) = spans[b][p]:
 *     a span with first < 0 or last < first is EMPTY: the token is bad and frees nothing;
 *     of any other span both ends are clamped into [0, n - 1] before anything is indexed, len = last - first + 1 of the clamped ends;
 *     such a token is bad iff len > max_span, or no frame f in [first, last] has mass[b][f][p] >= tau_tok (one fp32 comparison: a value
 *     equal to the threshold attends, a NaN never does);
 *     a bad token with a non-empty span frees the frames [max(0, first - margin), min(n - 1, last + margin)].
 * -> pin u8 (B,N): pin[b][f] = 1 for f < n that no bad token frees, and for f < n with keep[b][f] != 0 whatever the plan says; 0 for
 * every other f < N (every byte of the row is written).  counts i32 (B,2) = (bad tokens, frames f < n with pin 0).  A row with n == 0
 * or p1 <= p0 gets pin all 0 and counts (0, 0).  No index leaves the row whatever the buffers hold.  1 <= N <= 225, 1 <= P <= 198,
 * 1 <= B <= 65536, 1 <= max_span <= 225, 0 <= margin <= 32, tau_tok not NaN.
 *
 * smtts_repair_keep, 1 <= G <= 65535: with key(t) = isnan(t) ? +inf : t,
 *     replace[g] = counts[g][1] > 0 && key(total_new[g]) < key(total_cur[g])        (strict <: a tie keeps the current row, and a row
 *                                                                                    with nothing freed is never replaced)
 * Where replace[g] holds, row g of x_new f32 (G,N,64) and, where given, spans_new i32 (G,P,2) and mass_new f32 (G,N,P) is copied over
 * row g of x_cur, spans_cur, mass_cur IN PLACE, bit for bit (16-byte lanes where a row's byte count and both base addresses allow,
 * 4-byte elements otherwise: no alignment is required); every other row of the _cur buffers keeps its bits.  total_out f32 (G) and
 * feat_out i32 (G,4) are total / feat of whichever row stays, kept i32 (G) = replace.  counts i32 (G,2) is smtts_repair_plan's, feat_cur
 * / feat_new i32 (G,4) smtts_take_scores'.  spans_cur / spans_new and mass_cur / mass_new are each given or NULL together; a NULL pair
 * is skipped.  Every workgroup re-derives replace[g] from the inputs, so total_out, feat_out and kept must not overlap any input; the
 * _new buffers must not overlap the _cur ones.
 *
 * Both: an argument error (NULL handle or required pointer, half an optional pair, a shape or parameter out of range, a NaN threshold)
 * returns 1 with a message naming the entry before anything is enqueued.  One launch each, no atomics, no synchronisation: two calls
 * return the same bits.
 * Only this mechanism is verified.  It is UNVALIDATED on trained weights: every weight this project has run is seeded noise, nobody has
 * measured whether a 4-step distilled student inpaints the freed frames audibly well, nobody has measured whether a lower total is the
 * better take, and the thresholds the Python side passes by default (api.Repair) are design choices and not measurements. */
int smtts_repair_plan(smtts_handle h, void* stream, const float* mass, const int32_t* spans, const int32_t* n_len, const int32_t* p0,
                      const int32_t* p1, const uint8_t* keep /* or NULL */, int B, int N, int P, float tau_tok, int max_span, int margin,
                      uint8_t* pin, int32_t* counts);
int smtts_repair_keep(smtts_handle h, void* stream, int G, int N, int P, const float* total_cur, const float* total_new,
                      const int32_t* counts, const int32_t* feat_cur, const int32_t* feat_new, float* x_cur, const float* x_new,
                      int32_t* spans_cur /* or NULL */, const int32_t* spans_new, float* mass_cur /* or NULL */, const float* mass_new,
                      float* total_out, int32_t* feat_out, int32_t* kept);

/* ---- CTC score (DESIGN.md '8i. CTC score'): the latent phoneme recogniser and its CTC on the device -------------------------------
 * smtts_asr_logprobs replaces the reference's ASR(64).forward (src/smalltts/models/asr.py:41-52: upsample x4, a 7-layer Conformer at
 * width 64 with 16 heads, FFN 1024 and depthwise kernel 9, Linear 64 -> 198, log-softmax) for an engine that was given the asr.* tensors
 * (smtts_has_part(h, 3)).  x f32 (B,N,64) latents, n_len i32 (B) frames per row (clamped into [0, N]), both DEVICE -> logp f32
 * (B, 4 N, 198).  Row b has t_b = 4 n_b frames; every row is computed as if it were alone in its batch (attention keys and depthwise-conv
 * taps outside [0, t_b) do not exist), so nothing behind n_len[b] of x reaches a result, and logp at and behind frame t_b is written as
 * 0.0.  fp32 operands and accumulation; no atomics: two runs, alone or inside any batch, return the same bits.  ws: at least
 * smtts_asr_workspace_bytes(h, B, N) bytes, 256-byte aligned, contents irrelevant; x, n_len, logp 4-byte aligned.  1 <= B <= 64 and
 * 1 <= N <= 225, anything else (and an engine without the part) is an error; the size query returns 0 outside the range.
 *
 * smtts_ctc_score replaces CTCLoss(blank = 0) of the reference's distillation loss (src/scripts/train/dmd2/distill.py:344-348) as a
 * score: logp f32 (B,T,C), t_len i32 (B) (clamped into [0, T]), tokens i32 (B,P), p0 / p1 i32 (B) (clamped into [0, P] exactly as
 * smtts_align_path clamps them), all DEVICE.  The target of row b is tokens[b][p0 : p1), L = p1 - p0, every token clamped into [1, C) so
 * that no index leaves the row.  -> nll f32 (B) = F.ctc_loss(reduction = 'none', zero_infinity = False) of the row: the forward
 * recursion over the 2 L + 1 extended states in fp32, logaddexp with the maximum taken first (-inf, never NaN, when all operands are
 * -inf).  +inf for t_len == 0, for L <= 0 and for an infeasible row (t_len < L + repeats); a NaN that the recursion reads gives NaN.
 * 1 <= B <= 65536, 1 <= T <= 65536, 1 <= P <= 198, 2 <= C <= 256.  Needs no weights: works on any handle.
 *
 * smtts_ctc_greedy: per frame t < t_len[b] the class with the largest logp (the lowest class on ties; NaN is never the largest), equal
 * neighbours collapsed, class 0 dropped -> ids i32 (B,T) with zeros behind the count, n_ids i32 (B).  1 <= T <= 4096.  Any handle.
 * All three: one stream, no synchronisation, an argument error enqueues nothing. */
size_t smtts_asr_workspace_bytes(smtts_handle h, int B, int N);
int smtts_asr_logprobs(smtts_handle h, void* stream, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes,
                       float* logp);
int smtts_ctc_score(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                    const int32_t* p1, int B, int T, int P, int C, float* nll);
int smtts_ctc_greedy(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, int B, int T, int C, int32_t* ids,
                     int32_t* n_ids);

/* ---- Forced alignment (DESIGN.md '8l. Forced alignment'): the best path of smtts_ctc_score's lattice ------------------------------
 * smtts_ctc_align: logp, t_len, tokens, p0, p1 exactly as smtts_ctc_score takes and clamps them (t_len into [0, T], p0 / p1 into [0, P],
 * every token into [1, C)), all DEVICE.  Row b: target l = tokens[b][p0 : p1), L = p1 - p0, extended states [blank, l_0, blank, l_1, ...,
 * blank], S = 2 L + 1, label(s) = blank for even s and l_(s / 2) for odd s, T_b = t_len[b], lp_t = logp[b][t].  The definition, every step
 * a single fp32 operation:
 *     delta_0[0] = lp_0[0];  delta_0[1] = lp_0[l_0];  -inf elsewhere
 *     v = delta_{t-1}[s], m = 0
 *     if s >= 1  and delta_{t-1}[s-1] > v:  v = delta_{t-1}[s-1], m = 1
 *     if skip(s) and delta_{t-1}[s-2] > v:  v = delta_{t-1}[s-2], m = 2      (skip(s) = s odd, s >= 3 and label(s) != label(s - 2))
 *     delta_t[s] = v + lp_t[label(s)];  move_t[s] = m
 *     e = (delta_{T_b-1}[S-2] > delta_{T_b-1}[S-1]) ? S-2 : S-1
 *     score = delta_{T_b-1}[e]
 * The comparisons are strict: ties prefer staying, then one step; a NaN is never greater.  A row is ALIGNED iff score > -inf.  It is not
 * for t_len == 0 and L <= 0 (score = -inf), for an infeasible row (t_len < L + repeats: -inf) and for a NaN score; then every span is
 * (-1, -1), tok_logp is 0 and frame_tok is -1, and score is as computed.  An aligned row is traced back:
 *     s = e;  for t = T_b - 1 ... 1:  state[t] = s;  s = max(s - move_t[s], 0);   state[0] = s
 * (a bounded loop whose index stays in [0, S) whatever the data hold).  ->
 *   spans    i32 (B,P,2)  (first, last) frame t with state[t] == 2 (p - p0) + 1 for token p of [p0, p1), (-1, -1) for every other token;
 *   tok_logp f32 (B,P)    the sum of lp_t[label] over those frames, t ascending, single fp32 adds; 0 outside the window;
 *   frame_tok i32 (B,T)   optional (NULL: skipped): the token index p on a label frame, -1 on a blank frame and at or behind t_len[b];
 *   score    f32 (B).
 * Frames are frames of logp: behind smtts_asr_logprobs that is a quarter of a codec frame, 800 samples at 24 kHz.  One workgroup per
 * row and one launch; the 2-bit moves live in LDS (one 32-bit word per state and 16 steps, about 100 KB at the limits), so the trace
 * never leaves the CU and the entry takes no workspace.  Every sum has a fixed order and there are no atomics: two runs, alone or inside
 * any batch, return the same bits; nothing at or behind t_len[b] of a row, and nothing outside the row, is read.
 * 1 <= B <= 65536, 1 <= T <= 1024, 1 <= P <= 198, 2 <= C <= 256.  Needs no weights: works on any handle.  One stream, no
 * synchronisation; an argument error returns 1 with a message naming the entry before anything is enqueued.
 * Only this mechanism is verified.  As for the whole of 8i: no recogniser checkpoint has ever been loaded and the Conformer composition
 * is restated from recollection, so what an alignment of real speech is worth is UNVALIDATED. */
int smtts_ctc_align(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                    const int32_t* p1, int B, int T, int P, int C, int32_t* spans, float* tok_logp, int32_t* frame_tok /* or NULL */,
                    float* score);

/* ---- Long alignment (DESIGN.md '8m. Long alignment'): smtts_ctc_align for recordings past 30 s -------------------------------------
 * smtts_ctc_align_long: the definition is smtts_ctc_align's block above, word for word: the same clamping of t_len, p0, p1 and of every
 * token, the same recursion of single fp32 operations with strict compares, the same end rule and "ALIGNED iff score > -inf", the same
 * bounded trace, the same four outputs with the same values on a row that is not aligned.  Wherever both entries accept a call their
 * outputs are equal bit for bit.  What differs is where the lattice lives: one workgroup per row, every thread keeps delta of 32
 * neighbouring extended states in registers, the 2-bit moves go to the workspace (one 8-byte word pair per thread and step) and the
 * trace reads them back through LDS in chunks of 256 steps; the state of every frame goes to the workspace too.
 * ws: at least smtts_ctc_align_long_workspace_bytes(h, B, T, P) bytes = B * (align256(8 T ceil((2 P + 1) / 32)) + align256(2 T)), a
 * multiple of 256 (512 MiB + 128 KiB per row at the limits), 256-byte aligned, contents irrelevant on entry: every byte the kernel
 * reads it wrote in the same call.  The size query returns 0 outside the range.  Every output element of every row is written; nothing
 * at or behind t_len[b] of a row of logp, and nothing outside the row, is read; no atomics: two runs, alone or inside any batch, return
 * the same bits.
 * 1 <= B <= 64, 1 <= T <= 65536 (36 min of recogniser frames), 1 <= P <= 16383 (S = 2 P + 1 <= 32767), 2 <= C <= 256.  Needs no
 * weights: works on any handle.  One launch on one stream, no synchronisation; an argument error (a limit, a NULL required pointer, a
 * workspace that is NULL, misaligned or too small) returns 1 with a message naming the entry before anything is enqueued.
 * UNVALIDATED exactly as smtts_ctc_align: only the mechanism is verified. */
size_t smtts_ctc_align_long_workspace_bytes(smtts_handle h, int B, int T, int P);
int smtts_ctc_align_long(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                         const int32_t* p1, int B, int T, int P, int C, int32_t* spans, float* tok_logp, int32_t* frame_tok /* or NULL */,
                         float* score, void* ws, size_t ws_bytes);

/* ---- Speaker score (DESIGN.md '8j. Speaker score'): the latent speaker verifier on the device ---------------------------------------
 * smtts_sv_embed replaces the reference's SV(192).forward (src/smalltts/models/sv/model.py:26-35: speechbrain's ECAPA_TDNN on the 64-dim
 * latents, lengths / max as its relative lengths) for an engine that was given the sv.* tensors (smtts_has_part(h, 4)).  x f32 (B,N,64)
 * latents, n_len i32 (B) frames per row (clamped into [0, N]), both DEVICE -> emb f32 (B, 192), not normalised.  Every row is computed
 * as if it were alone in its batch at its own length: reflect padding reflects about the row's own first and last frame and every mean,
 * softmax and statistic runs over [0, n_b), so nothing at or behind n_len[b] of x reaches a result (what the reference computes for a
 * batch of one).  A row with n_b < 6 has no embedding (the dilation-5 reflect padding needs more frames than it pads): its emb row is
 * written as 0.0.  fp32 operands and accumulation; no atomics: two runs, alone or inside any batch, return the same bits.  ws: at least
 * smtts_sv_workspace_bytes(h, B, N) bytes, 256-byte aligned, contents irrelevant; x, n_len, emb 4-byte aligned.  1 <= B <= 64 and
 * 6 <= N <= 225, anything else (and an engine without the part) is an error; the size query returns 0 outside the range.
 *
 * smtts_sv_cosine replaces cosine_loss's similarity of the reference's distillation loss (src/scripts/train/dmd2/distill.py:30-31,
 * 351-353) as a score: row b of emb f32 (B,D) against row b / K of ref f32 (B/K,D), both DEVICE -> cos f32 (B) =
 * (a . r) / (max(||a||, 1e-8) max(||r||, 1e-8)), F.cosine_similarity's rule: a zero row gives 0.  1 <= B <= 65536, 1 <= K <= 16,
 * B % K == 0, 1 <= D <= 1024.  Needs no weights: works on any handle.
 * Both: one stream, no synchronisation, an argument error enqueues nothing.
 * Limits: the score is unvalidated on trained weights (every weight this project has run is seeded noise); the ECAPA composition and
 * its state-dict names are restated from recollection, unpinned; no verifier checkpoint has ever been loaded. */
size_t smtts_sv_workspace_bytes(smtts_handle h, int B, int N);
int smtts_sv_embed(smtts_handle h, void* stream, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes,
                   float* emb);
int smtts_sv_cosine(smtts_handle h, void* stream, const float* emb, const float* ref, int B, int K, int D, float* cos);

/* ---- codec ------------------------------------------------------------------------------------ */
int smtts_codec_hop(smtts_handle h);
size_t smtts_decode_workspace_bytes(smtts_handle h, int B, int T);
/* latents f32 (B,T,64) -> audio f32 (B,1,hop*T) */
int smtts_codec_decode(smtts_handle h, void* stream, const float* latents, int B, int T, float* audio, void* ws,
                       size_t ws_bytes);
/* ---- streamed decode: chunks of audio with carried causal state (DESIGN.md '8f. Streamed decode') ------------------------------
 * smtts_codec_decode_stream decodes the next T latent frames of B independent streams and returns their hop * T samples each; the
 * concatenation of a stream's chunks is the decode of the concatenated latents (the same kernels as smtts_codec_decode, chosen by the
 * same gates at the chunk's B and T; fp32 summation order is the only admissible difference where a gate picks another kernel at
 * another size).  Nothing in the codec depends on absolute position and no kernel looks back further than 6 frames, so a stream's
 * whole memory is, for every image a look-back kernel reads, the last 8 frames that image had: its STATE.
 *
 * State pool: caller-owned DEVICE memory, n_slots slots of smtts_decode_state_bytes(h) bytes each (the slot stride; a multiple of 256),
 * 16-byte aligned.  A slot holds one [8][C] fp32 block per boundary, densely in this order (the size is their sum, rounded up to 256):
 *     the latent image (C = latent_dim); the input of every block of every stage, stages and blocks in decoder order (C of the stage);
 *     the output of every stage that feeds a ConvTranspose, in stage order; the head's input (C of the last stage).
 * Default spec: 34 boundaries, 849 920 bytes.  Frame j of a block is the frame 8 - j steps before the next frame of that image.
 * A ZERO slot is the start of an utterance (the causal zero padding): smtts_codec_decode_stream on a zeroed slot returns what
 * smtts_codec_decode returns, bit for bit.  After a chunk of T >= 8 frames a block holds the image's last 8 frames; after T < 8 the old
 * block moved up by T frames with the chunk's T frames behind it.  The state belongs to the caller between calls: copying a slot
 * (device to device, ordered against the calls on their stream) takes a snapshot a stream can be rewound to, zeroing it resets the
 * stream.  It depends on the weights and the codec spec, not on precision or tuning.
 * slots: DEVICE int64 (B), the slot of every row (smtts_voice_expand's table convention); a slot may appear at most ONCE per call (two
 * rows on one slot race).  The table is not visible to the host side of this call: the kernel clamps every index into [0, n_slots),
 * it never follows one outside the pool.  ws: smtts_decode_stream_workspace_bytes(h, B, T) bytes, 256-byte aligned: the plan of
 * smtts_codec_decode at the CHUNK's size, whatever the utterance's length.
 * Refused with an error, nothing enqueued: no finalized decoder, B < 1, T < 1, n_slots < 1, a NULL pointer, a pool that is not 16-byte
 * aligned, a workspace that is too small or not 256-byte aligned.  One launch (carry_frames) per boundary and chunk more than
 * smtts_codec_decode, none of its pad-zeroing launches. */
size_t smtts_decode_state_bytes(smtts_handle h);                       /* per slot, multiple of 256; 0 on error */
size_t smtts_decode_stream_workspace_bytes(smtts_handle h, int B, int T);
int smtts_codec_decode_stream(smtts_handle h, void* stream, const float* latents, int B, int T, void* state_pool, int64_t n_slots,
                              const int64_t* slots /* DEVICE (B) */, float* audio /* (B,1,hop*T) */, void* ws, size_t ws_bytes);
size_t smtts_encode_workspace_bytes(smtts_handle h, int B, int S);
/* audio f32 (B,1,S) -> latents f32 (B, S/hop, 64) */
int smtts_codec_encode(smtts_handle h, void* stream, const float* audio, int B, int S, float* latents, void* ws,
                       size_t ws_bytes);

/* ---- utilities -------------------------------------------------------------------------------- */
/* standard normals, same generator the sampler uses: element i <- Philox4x32-10(counter=(i/4, stream_id), key=seed) */
int smtts_randn(smtts_handle h, void* stream, float* out, int64_t n, uint64_t seed, uint64_t stream_id);
/* (alpha, sigma) of the reference schedule for t (infer/onnx.py:31-39); host-side, float64 math */
void smtts_alpha_sigma(float t, float* alpha, float* sigma);

/* ---- device-side audio front / back end -----------------------------------------------
 * Polyphase windowed-sinc resampling of `channels` rows of n_in samples (reference infer/utils.py:7-16, torchaudio
 * Resample with sinc_interp_kaiser): y[c][f*up + p] = sum_k xpad[c][f*down + k] * bank[p][k], xpad = x with `width`
 * leading zeros.  The caller builds the bank [up][klen] (smalltts_amd/audio.py:_sinc_kernel) and owns every buffer. */
int smtts_resample_poly(smtts_handle h, void* stream, const float* x, int channels, int64_t n_in, const float* bank, int up,
                        int down, int klen, int width, float* y, int64_t n_out);
/* float [-1, 1] -> int16 PCM: clamp, x 32767, round to nearest (reference server audio.rs:22-37; CLIs write PCM_16, tryme.py:29) */
int smtts_pcm16(smtts_handle h, void* stream, const float* x, int64_t n, int16_t* y);

/* ---- delivery: audio at the caller's rate and encoding, whole or streamed (DESIGN.md '8g. Delivery') ------------------------------
 * smtts_deliver resamples the next chunk of B independent streams with a polyphase bank and encodes the result; the concatenation
 * of a stream's chunks is, BIT FOR BIT, the delivery of the whole signal in one call, whatever the chunking.  Additive entries.
 *
 * Signal: audio f32 (B,1,row_stride), DEVICE.  table: DEVICE int64 (B,4) = (slot, n_before, len, last) per row: row b of this call is
 * the next len[b] samples (clamped to [0, row_stride]; nothing behind them is read) of a stream that has already seen n_before[b]
 * samples (clamped to [0, 2^50]); last != 0: the stream ends with this chunk.  x = the stream's whole signal, n = n_before + len.
 * Bank: f32 [up][klen], klen = 2 * width + down, the layout of smtts_resample_poly (smalltts_amd/audio.py:_sinc_kernel).
 * Sum:  y[f * up + p] = sum_{k = 0 .. klen - 1} x[f * down - width + k] * bank[p][k], where x[i] enters as +0.0f for i < 0 and,
 *       once the stream has ended, for i >= n.  Every sample is ONE chain acc = fmaf(x_k, bank[p][k], acc) from acc = +0.0f over ALL
 *       klen taps in the order k = 0 .. klen - 1 (no sum is shortened at an edge), in whichever call it is emitted.
 *       n_before = 0, len = n, last = 1 is smtts_resample_poly's definition cut to ceil(up * n / down) samples (audio.resample_hq's
 *       length).
 * Emission: F(m) = max(0, (m - width) / down) (integer division) = the frames all of whose inputs lie in x[0 .. m).
 *       last == 0: row b writes the frames [F(n_before), F(n)), up * (F(n) - F(n_before)) samples;
 *       last != 0: the samples [up * F(n_before), ceil(up * n / down)).
 *       They go to out[b][0 .. cnt_b), nothing is written behind them.  len = 0 with last != 0 is a pure flush.  The host knows
 *       cnt_b from integers alone (smalltts_amd/audio.py:deliver_counts).
 * State: caller-owned DEVICE pool of n_slots slots of smtts_deliver_state_bytes(h, klen) bytes each (the slot stride, a multiple of
 *       256), 16-byte aligned.  A slot holds the stream's last H = klen - 1 input samples as f32, oldest first; a ZERO slot is the
 *       start of a stream.  After the call the slot holds the last H samples of x[0 .. n) (with len < H the old content moves up by
 *       len), also after last != 0.  slot indices are clamped into [0, n_slots) by the kernel, never followed outside the pool; a
 *       slot may appear at most ONCE per call (smtts_codec_decode_stream's rules; the Python wrapper refuses duplicates and indices
 *       out of range).  The slot belongs to the caller between calls: copy it for a snapshot, zero it to reset the stream.
 *       The history is updated by a second launch (one workgroup per row: loads, a barrier, stores) behind the main one.
 *       state_pool == NULL with a bank: every row starts and ends here: history reads as zeros, nothing is carried, slot is ignored,
 *       and every row must have n_before = 0 and last = 1 (the kernel reads them as such).
 * Pass-through: up == down == 1 with bank == NULL, klen == width == 0 and state_pool == NULL is the native rate: a pure encode with
 *       no state, F(m) = m, cnt_b = len[b] whatever `last` says.
 * enc:  0 = f32;  1 = int16, exactly smtts_pcm16's arithmetic on the f32 value (clamp to [-1, 1], x 32767, round to nearest even);
 *       2 = G.711 mu-law (uint8) of that int16 s;  3 = G.711 A-law (uint8) of that int16 s.  The codes are byte for byte those of
 *       CPython's audioop.lin2ulaw(s, 2) / audioop.lin2alaw(s, 2), i.e. the CCITT / Sun g711.c encoders on s >> 2 and s >> 3
 *       (arithmetic shifts).  With seg(v, e) = the number of i in 0 .. 7 with v > (e + 1) * 2^i - 1:
 *         mu-law: v = s >> 2; mask = 0xFF; if v < 0: v = -v, mask = 0x7F; v = min(v, 8159) + 33; g = seg(v, 0x3F);
 *                 code = g >= 8 ? 0x7F ^ mask : ((g << 4) | ((v >> (g + 1)) & 15)) ^ mask
 *         A-law:  v = s >> 3; mask = 0xD5; if v < 0: v = -v - 1, mask = 0x55; g = seg(v, 0x1F);
 *                 code = g >= 8 ? 0x7F ^ mask : ((g << 4) | ((v >> (g < 2 ? 1 : g)) & 15)) ^ mask
 *       Known answers (s: mu-law, A-law): 0: ff d5; 1: ff d5; -1: 7e 55; 4: fe d5; -4: 7e 55; 100: f2 d3; -100: 72 53;
 *       1000: ce fa; -1000: 4e 7a; 32635: 80 aa; 32767: 80 aa; -32768: 00 2a.
 *       out_stride (the row pitch of out) counts elements of the output type.
 * Refused with 1 and a message naming the entry, nothing enqueued: a NULL handle (the size query returns 0); B outside [1, 65535];
 *       row_stride outside [1, 2^40]; a NULL audio, table or out; up or down outside [1, 4096]; with a bank: klen != 2 * width + down,
 *       klen > 8192, a tile window of (256 / up + 1) * down + klen floats plus a bank of up to 48 KiB above 64 KiB of LDS; without a
 *       bank anything but the pass-through form; a pool with klen <= 1, with n_slots < 1 or not 16-byte aligned; enc outside 0 .. 3;
 *       out_stride smaller than the largest count row_stride can produce: ceil(up * (row_stride + width + down - 1) / down) with a
 *       pool, ceil(up * row_stride / down) without, row_stride at the pass-through rate.
 * One launch whatever B is, plus the history launch when a pool is given.  No atomics, nothing depends on scheduling: two calls return
 * the same bits.
 * Only this mechanism is verified.  The banks the Python side builds (audio._sinc_kernel: a Kaiser-windowed sinc restated from
 * torchaudio's published algorithm) are unpinned against torchaudio, as on the input side, and their 64 zero crossings
 * (audio.DELIVER_ZEROS) are a design choice, not a measurement. */
size_t smtts_deliver_state_bytes(smtts_handle h, int klen);   /* per slot, multiple of 256; 0 for klen <= 1 or on error */
int smtts_deliver(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride,
                  const int64_t* table /* DEVICE (B,4): slot, n_before, len, last */, const float* bank, int up, int down, int klen,
                  int width, void* state_pool, int64_t n_slots, int enc, void* out, int64_t out_stride);

/* ---- watermark: key the 24 kHz stream on the device, detect it (DESIGN.md '8k. Watermark') ----------------------------------------
 * A zero-bit, keyed, additive spread-spectrum mark.  The mark is a function of the ABSOLUTE stream position, so the concatenation of a
 * stream's marked chunks is, BIT FOR BIT, the mark of the whole signal in one call, whatever the chunking.  Additive entries.
 *
 * Chips: for stream sample i >= 0, w = the four words of Philox4x32-10 with counter (lo32(i >> 7), hi32(i >> 7), 0x574D4B31, 0) and
 *       key (lo32(key), hi32(key)) (smtts_randn's counter layout with stream id 'WMK1'; oracle/philox.py restates it).
 *       c[i] = +1 if bit (i & 31) of w[(i >> 5) & 3] is set, else -1.
 *
 * smtts_watermark
 * Signal: audio, out f32 (B,1,row_stride), DEVICE, not overlapping.  table: DEVICE int64 (B,4) = (slot, n_before, len, last) with
 *       smtts_deliver's clamps (len to [0, row_stride], n_before to [0, 2^50], slot into the pool); `last` is ignored: there is no
 *       look-ahead.  x = the stream's whole signal so far, row b of this call = x[n_before .. n_before + len).
 * Mark: block k = the samples [64 k, 64 k + 64).  E[k] = ONE sequential fp32 chain over j = 0 .. 63 from acc = +0.0f:
 *       sq = x_j * x_j (rounded), acc = acc + sq (rounded); no fma.  R[k] = sqrt(E[k] * 0.015625f) (correctly rounded).
 *       A[k] = strength * R[k - 1] (one rounded multiply), A[0] = 0.
 *       y[i] = c[i] > 0 ? x[i] + A[i / 64] : x[i] - A[i / 64]: one rounded fp32 add; no clamp (the encoders clamp).
 *       So silence stays silence, the first block is never marked, strength = 0 changes no value (-0.0f + 0.0f is +0.0f: a zero's
 *       sign may change, nothing else), and a numpy float32 loop reproduces y exactly.
 *       Row b writes out[b][0 .. len_b) and nothing behind that.
 * State: caller-owned DEVICE pool of n_slots slots of smtts_watermark_state_bytes(h) = 512 bytes each, 16-byte aligned.  A slot holds
 *       the stream's last 127 INPUT (unmarked) samples as f32, oldest first (127 f32, rounded up to 512 bytes); a ZERO slot is the
 *       start of a stream.  After the call the slot holds the last 127 samples of x[0 .. n_before + len) (with len < 127 the old
 *       content moves up by len).  It is updated by a second launch (one workgroup per row: loads, a barrier, stores) behind the
 *       main one.  Slot indices are clamped, never followed outside the pool; a slot may appear at most ONCE per call (the Python
 *       wrapper refuses duplicates).  state_pool == NULL: every row starts here: n_before reads as 0, slot is ignored, nothing is
 *       carried.
 * Refused with 1 and a message naming the entry, nothing enqueued: a NULL handle (the size query returns 0), audio, table or out;
 *       B outside [1, 65535]; row_stride outside [1, 2^40]; strength negative, not finite or above 1; audio and out overlapping (in
 *       place is a race on the block in front); a pool with n_slots < 1 or not 16-byte aligned.
 * One launch whatever B is, plus the history launch when a pool is given.  No atomics: two calls return the same bits.
 *
 * smtts_watermark_detect
 * Signal: audio f32 (B,row_stride), DEVICE; len DEVICE int64 (B), clamped to [0, row_stride]; nothing behind len is read.  y = the
 *       row's len samples, zeros outside [0, len).  The device works in fp32.
 *       d2[j] = y[j-1] - 2 y[j] + y[j+1] for 0 <= j < len, 0 outside;   d4[j] = y[j-2] - 4 y[j-1] + 6 y[j] - 4 y[j+1] + y[j+2];
 *       r[j] = sqrt((1/64) sum_{m = j-96 .. j-33} y[m]^2);   v[j] = (1/64) sum_{m = j-32 .. j+31} d2[m]^2;
 *       u[j] = d4[j] * r[j] / (v[j] + 1e-8f);   den = sum_{j < len} u[j]^2.
 *       For offset o (audio[j] is stream sample j + o): T(o) = sum_{j < len} u[j] * c[j + o], z(o) = T(o) / sqrt(den).
 *       u does not depend on o.  Under "not marked with this key" z(o) is about N(0, 1).
 * Order: u[j]: d2 = (y[m-1] + y[m+1]) - 2 y[m]; both 64-term sums are chains in ascending m from +0.0f; the square root and the
 *       division are correctly rounded; d4 = ((y[j-2] + y[j+2]) - 4 (y[j-1] + y[j+1])) + 6 y[j]; u = (d4 * r) / (v + 1e-8f).  No
 *       product is contracted into the sum behind it (a contraction would only remove roundings).
 *       T(o): tiles of 1024 samples in ascending order; inside a tile a chain acc = acc + (+-u[j]) in ascending j from +0.0f (the
 *       sign flipped exactly, no product), then ONE add total = total + acc, total from +0.0f.
 *       den: per tile of 1024 samples thread t (of 256) chains u[t]^2, u[t + 256]^2, u[t + 512]^2, u[t + 768]^2 (0 at or behind len)
 *       from +0.0f, then a halving tree (stride 128, 64 .. 1: s[t] += s[t + stride]); over the ceil(len / 1024) tile sums the same
 *       again: thread t chains the tiles t, t + 256, ..., then the same tree.
 *       So two calls return the same bits and a row does not depend on its batch-mates.
 * Out, all DEVICE: u f32 (B,row_stride), written below len only; may be NULL, it then lives in ws.  den f32 (B).  T f32 (B,n_off),
 *       T[b][k] = T(o_lo + k).  best_off int64 (B) = o_lo + argmax_k T[b][k], the lowest k on ties.  best_z f32 (B) =
 *       T[b][best] / sqrtf(den[b]) (both correctly rounded), 0 where den[b] == 0.
 * Workspace: smtts_watermark_detect_workspace_bytes(h, B, row_stride) bytes, 256-byte aligned: u's place and the tile sums.
 * Refused with 1 and a message naming the entry, nothing enqueued: a NULL handle (the size query returns 0); B outside [1, 1024];
 *       row_stride outside [1, 2^40]; a NULL audio, len, ws, den, T, best_off or best_z; o_lo outside [0, 2^40]; n_off outside
 *       [1, 65536]; a workspace not 256-byte aligned or smaller than the query's answer.
 * Three launches whatever B, len and n_off are.  Needs no weights: works on any handle, like smtts_sv_cosine.
 * Unvalidated: detection on real speech and on trained weights; the default strength has never been listened to. */
size_t smtts_watermark_state_bytes(smtts_handle h);   /* per slot: 512 */
int smtts_watermark(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride,
                    const int64_t* table /* DEVICE (B,4): slot, n_before, len, last */, uint64_t key, float strength,
                    void* state_pool, int64_t n_slots, float* out);
size_t smtts_watermark_detect_workspace_bytes(smtts_handle h, int B, int64_t row_stride);
int smtts_watermark_detect(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len /* DEVICE (B) */,
                           uint64_t key, int64_t o_lo, int n_off, void* ws, size_t ws_bytes, float* u, float* den, float* T,
                           int64_t* best_off, float* best_z);

/* ---- long-form synthesis: one voice, many rows (DESIGN.md 'Long-form synthesis') ----------------------------------
 * The two halves of smtts_cond_encode are independent (k_ref / v_ref depend on the reference only, k_text / v_text on the phonemes
 * only; reference model.py:88-95, dit.py:80-93) and a half whose length is 0 is skipped: R = 0 with ref / ref_len / k_ref / v_ref /
 * ref_mask NULL encodes the text half alone, P = 0 with phonemes / ph_mask / k_text / v_text NULL the voice half alone.  A voice is
 * therefore encoded ONCE at B = 1, P = 0 and handed to every later batch:
 * smtts_voice_expand gathers per-voice slabs into the batch cache smtts_sample / smtts_denoise_step take.  table: DEVICE int64
 * [B][3] = (k_ptr, v_ptr, R_b), the device addresses of a voice's k_ref / v_ref (12,1,8,R_b,120) f32 as smtts_cond_encode(B = 1)
 * wrote them; the same voice may appear in many rows.  -> k_ref, v_ref f32 (12,B,8,Rmax,120), ref_mask bool (B,Rmax): positions
 * j < R_b are bit-identical copies and masked true, positions j >= R_b are zero and masked false (R_b is clamped to [0, Rmax]).
 * One launch whatever B is; the slabs are read on `stream`, so they must stay alive and unchanged until that work has completed. */
int smtts_voice_expand(smtts_handle h, void* stream, const int64_t* table, int B, int Rmax, float* k_ref, float* v_ref,
                       uint8_t* ref_mask);
/* per-row sampler noise in one launch: out f32 (n_steps,B,Nmax,64); row b of step s holds in [0, n[b] * 64) exactly what
 * smtts_randn(n = n[b] * 64, seed = seeds[b], stream_id = s) writes, zeros behind (n[b] is clamped to [0, Nmax]) — a row's noise does
 * not depend on its batch-mates.  seeds u64 (B) and n i64 (B) are DEVICE arrays. */
int smtts_randn_rows(smtts_handle h, void* stream, float* out, const uint64_t* seeds, const int64_t* n, int n_steps, int B,
                     int Nmax);
/* joins rows of a decoded batch into one waveform: audio f32 (B,1,row_stride); len, off i64 (B) DEVICE arrays (samples of row b, its
 * absolute offset in out); fade f32 (F) DEVICE table (F = 0: none, fade may be NULL).  For i < len[b]: out[off[b] + i] = audio[b][i] * g,
 * F_b = min(F, len[b] / 2), g = fade[i] for i < F_b, fade[len[b] - 1 - i] for i >= len[b] - F_b, otherwise no multiply.  out has out_n
 * elements: f32 (pcm16 = 0) or int16 (pcm16 != 0: smtts_pcm16's clamp, x 32767, round to nearest on the faded value).  Samples between
 * rows are not written (zero-fill out once); samples outside [0, out_n) are dropped; len[b] is clamped to row_stride.  Several batches
 * of one text write into the same out at different offsets.  One fp32 multiply by a table entry per sample: numpy reproduces it bit
 * for bit. */
int smtts_stitch(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, const int64_t* off,
                 const float* fade, int F, void* out, int64_t out_n, int pcm16);
/* endpoints of the speech in each row of a decoded batch: audio f32 (B,1,row_stride); len i64 (B) DEVICE (clamped to
 * [0, row_stride]; nothing behind len[b] is read); e, pk f32 (B,Fmax), Fmax = ceil(row_stride / W), scratch AND output: the per-frame
 * mean power and peak, written for f < ceil(len[b] / W), untouched behind; -> seg i64 (B,2) = (start, n), gain f32 (B), both DEVICE.
 *   frame f covers [f W, min(len, (f + 1) W)), cnt[f] samples; e[f] = (sum x^2) / cnt[f] (fp32, a fixed order), pk[f] = max |x|;
 *   thr = fmaxf(max_f e[f] * rel_pow, floor_pow); f is active iff e[f] > thr, speech iff it lies in a run of >= min_run active frames;
 *   no speech: (0, 0), gain 1.  Else with a / b the first / last speech frame: start = max(0, a W - lead),
 *   n = min(len, (b + 1) W + tail) - start;  gain = 1 if target_rms == 0, else P = (sum over speech frames of e[f] cnt[f]) / (sum of
 *   cnt[f]), g = fminf(target_rms / sqrtf(P), max_gain), and g = peak_limit / max_f pk[f] if max_f pk[f] * g > peak_limit.
 * Given the e returned, integer logic and single fp32 operations reproduce (start, n) exactly and gain up to the summation order of P.
 * Two launches whatever B is; no atomics: two calls on the same input return the same bits, and a row's results do not depend on its
 * batch-mates.  W % 4 == 0, 16 <= W <= 4096; 1 <= min_run <= 16; lead, tail >= 0; rel_pow, floor_pow, target_rms >= 0; peak_limit,
 * max_gain > 0. */
int smtts_endpoints(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, int W,
                    float rel_pow, float floor_pow, int min_run, int lead, int tail, float target_rms, float peak_limit,
                    float max_gain, float* e, float* pk, int64_t* seg, float* gain);
/* smtts_stitch with a source window and a gain per row: seg i64 (B,2) DEVICE = (start, n) as smtts_endpoints writes it (clamped into
 * [0, row_stride]), gain f32 (B) DEVICE or NULL, off i64 (B) DEVICE.  For i < n: out[off[b] + i] = ((audio[b][start + i] * gain[b]) * g),
 * g the fade weight of smtts_stitch over the window (F_b = min(F, n / 2)); each step is one fp32 multiply, gain == NULL skips the first
 * (it does not even round); then smtts_stitch's PCM16 arithmetic when pcm16 != 0.  seg = (0, len) with gain NULL is smtts_stitch. */
int smtts_stitch_seg(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* seg,
                     const float* gain, const int64_t* off, const float* fade, int F, void* out, int64_t out_n, int pcm16);
/* the running join: the joined stream of a long text as an APPEND, batch by batch, with the plan made on the device.
 * Stream: the pieces come in order, over any number of calls on one state; piece b of a call is the window (start, n) = seg[b] of its
 *       row, clamped into the row as smtts_stitch_seg clamps it (a negative n is 0).  A piece with n = 0 takes neither room nor a gap.
 *       A non-empty piece is preceded by `gap` samples of +0.0 if and only if a non-empty piece came before it, in this call or in any
 *       earlier call on the same state.  A sample of a window is ((audio[b][start + i] * gain[b]) * g), g the fade weight of
 *       smtts_stitch over the window's own ends (F_b = min(F, n / 2)); each step is one fp32 multiply, gain == NULL skips the first (it
 *       does not even round); then smtts_stitch's PCM16 arithmetic when pcm16 != 0 (a gap sample is then the int16 0).  This is what
 *       api.plan_packed and smtts_stitch_seg write into one zero-filled buffer; seg = (0, len) with every n > 0 is plan_long's layout.
 * State: caller-owned DEVICE slot of two int64, 16-byte aligned: pos = samples of the joined stream emitted so far, k = non-empty
 *       pieces so far.  A ZERO slot starts a stream.  It belongs to the caller between calls: copy it for a snapshot.
 * In:   audio f32 (B,1,row_stride); seg i64 (B,2) DEVICE (what smtts_endpoints left there: no host round trip); gain f32 (B) DEVICE or
 *       NULL; fade f32 (F) DEVICE (F = 0: none, fade may be NULL); gap >= 0 samples; last (copied into dtable only).
 * Out:  chunk[0 .. pos_after - pos_before), f32 or (pcm16 != 0) int16, chunk_cap elements: the next samples of the joined stream, the
 *       gaps included as zeros the kernel writes (no memset of the chunk); nothing behind the chunk's length is touched.  Samples that
 *       would land at or beyond chunk_cap are dropped; rec still carries the untruncated pos_after (sum of min(n_b, row_stride) + B *
 *       gap elements always suffice).
 *       off i64 (B) DEVICE: the ABSOLUTE position of piece b in the joined stream (an empty piece: where the last non-empty one ended,
 *       as plan_packed has it).
 *       rec i64 (4) DEVICE = (pos_before, pos_after, k_before, k_after).
 *       dtable i64 (4) DEVICE or NULL = (slot, n_before = pos_before, len = pos_after - pos_before, last != 0): exactly the row
 *       smtts_deliver reads, so a delivery of the chunk (B = 1, row_stride = chunk_cap) can be enqueued right behind without the host
 *       knowing the length; `slot` is copied through.
 * One main launch whatever B is: every workgroup derives its row's offset from the seg table and the slot itself (no prefix-sum
 *       launch, no atomics; integer sums, so their order cannot matter).  The state is advanced, and rec / dtable are written, by a
 *       second small launch behind the main one, so that no workgroup of the first sees a slot half written (smtts_deliver's history
 *       launch is the precedent).  Nothing depends on scheduling: two calls on equal inputs return equal bits.
 * Refused with 1 and a message naming the entry, nothing enqueued: a NULL handle, audio, seg, off, rec, chunk or state; a state that
 *       is not 16-byte aligned; B outside [1, 1024]; row_stride outside [1, 2^40]; gap < 0 or gap > 2^31; F < 0, or F > 0 with fade
 *       NULL; chunk_cap < 1. */
int smtts_join_stream(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* seg,
                      const float* gain, const float* fade, int F, int64_t gap, int last, int64_t* state /* DEVICE (2): pos, k */,
                      void* chunk, int64_t chunk_cap, int pcm16, int64_t* off, int64_t* rec, int64_t* dtable, int64_t slot);
/* retiming: time-scale modification of each row onto a table of (source, target) anchors by waveform-similarity
 * overlap-add (WSOLA): the output is built from segments of H = hop samples; a segment is taken from where the previous one would
 * have continued if that lies within D = delta samples of where the map says, else from the place within D of the map whose samples
 * correlate best with that continuation, cross-faded with it.  Pitch is kept; a unit map returns the input's bits.
 * In:   audio f32 (B,1,row_stride); len i64 (B) DEVICE; anchors i64 (B,A,2) DEVICE = (src, dst) sample positions; n_anchor i64 (B)
 *       DEVICE; win f32 (2 H) DEVICE, the cross-fade window: win[i] weights the new place, win[H + i] the continuation.
 * Samples: n = clamp(len[b], 0, row_stride); a source sample x[s] outside [0, n) reads as +0.0, and nothing behind n is loaded.
 * Map:  m = clamp(n_anchor[b], 0, A) anchors (s_j, d_j) are in use; every entry is clamped as it is loaded, s_j into
 *       [0, row_stride], d_j into [0, out_stride].  out_len = d_{m-1}; with m < 2 it is 0 and nothing is written.  For
 *       d_j <= t < d_{j+1}: M(t) = s_j + ((t - d_j) * (s_{j+1} - s_j)) // (d_{j+1} - d_j), int64, // rounding down; for t >= d_{m-1}
 *       (or where no pair is left): M(t) = s_{m-1} + (t - d_{m-1}); the result is clamped into [0, n].  M is evaluated at t = 0, H,
 *       2 H, ... in order and the pair index never moves back: from the pair the previous evaluation ended at it advances to the
 *       first j with d_{j+1} > d_j and d_j <= t < d_{j+1} (a pair with d_{j+1} <= d_j is skipped).  For a table with d_0 = 0 and
 *       increasing d this is the plain piecewise map; for any other contents it is still defined, and the kernel stays inside its
 *       buffers: the tables live on the device, so they are clamped, never trusted.
 * Segments: K = ceil(out_len / H); segment k covers out[k H, min((k + 1) H, out_len)).
 *       k = 0:  q_0 = M(0), out[i] = x[q_0 + i].
 *       k >= 1: p = M(k H), c = q_{k-1} + H.  If |c - p| <= D: q_k = c and out[k H + i] = x[c + i], a copy (no arithmetic).
 *               Else the lags l in [-D, D] with 0 <= p + l <= n are candidates (l = 0 always is one),
 *               score(l) = sum over i < H of x[c + i] * x[p + l + i] in fp32, in any order, with or without fma; a score that
 *               comes out NaN (NaN or Inf samples inside len) counts as -inf;
 *               q_k = p + l*, l* the lag of the largest score, on equal scores the smaller |l|, then the negative lag;
 *               q_k == c: the copy again; else out[k H + i] = fadd(fmul(x[c + i], win[H + i]), fmul(x[q_k + i], win[i])), three
 *               separately rounded fp32 operations (no fma), which numpy reproduces bit for bit given q.
 * Out:  out f32 (B,1,out_stride): row b holds out_len samples, nothing at or behind out_len is written; q i64 (B,Kmax) DEVICE or
 *       NULL, Kmax = ceil(out_stride / H): q[b][k] = q_k for k < K, nothing at or behind K is written.  audio and out must not
 *       overlap.
 * One launch whatever B is, one workgroup per row (the segments of a row are a chain); no atomics, nothing depends on scheduling:
 *       two calls on equal inputs return equal bits, and a row's results do not depend on its batch-mates.
 * Refused with 1 and a message naming the entry, nothing enqueued: a NULL handle, audio, len, anchors, n_anchor, win or out; B
 *       outside [1, 1024]; row_stride or out_stride outside [1, 2^31 - 1] (the map's products then fit int64); A outside [2, 65536];
 *       hop outside [16, 512] or not a multiple of 4; delta outside [0, 512]. */
int smtts_retime(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len /* DEVICE (B) */,
                 const int64_t* anchors /* DEVICE (B,A,2) */, const int64_t* n_anchor /* DEVICE (B) */, int A, const float* win,
                 int hop, int delta, float* out, int64_t out_stride, int64_t* q);
/* pitch: an F0 track of each row.  Every frame of hop samples gets a normalised cross-correlation score (NCCF) per
 * candidate lag, and the cheapest path through "unvoiced" and the lags (Viterbi, with a cost per octave of jump and per switch of
 * voicing) gives one lag, or 0 for unvoiced, per frame.  The constants are the caller's; the defaults of the Python side are design
 * choices checked on synthetic signals only, nothing here was tuned or validated on speech.
 * In:   audio f32 (B,1,row_stride); len i64 (B) DEVICE; tab f32 (2,L) DEVICE: lg[0..L) then tilt[0..L), L = lmax - lmin + 1
 *       (plans.pitch_tables: lg = log2 of the lag, tilt falls from 1 at lmin).  Every entry is clamped as it is loaded, lg into
 *       [0, 16], tilt into [0, 2], a NaN reads as 0: the table lives on the device, so it is clamped, never trusted.
 * Samples: n = clamp(len[b], 0, row_stride); x[i] outside [0, n) reads as +0.0, and nothing behind n is loaded.
 *       F_b = ceil(n / hop) frames; frame f starts at s = f * hop.  Fmax = ceil(row_stride / hop).
 * Scores for lag l in [lmin, lmax], column l - lmin:  r = sum_{i<win} x[s+i] * x[s+l+i],  e0 = sum_{i<win} x[s+i]^2,
 *       e = sum_{i<win} x[s+l+i]^2,  S[f][l] = r / sqrtf(e0 * e + bias).  Each sum is fp32, in any order, with or without fma; the
 *       product, the add, sqrtf and the divide are correctly rounded fp32 operations.  bias > 0 makes silence score 0 smoothly (no
 *       energy gate, no discrete decision on a rounded sum); the Python side passes (win * floor_pow)^2.  Silence scores exactly 0.
 * States: j = 0 is unvoiced, j = 1 .. L is lag lmin + j - 1.
 * Local cost, every named operation one separately rounded fp32 operation (no fma):  loc(f, 0) = c_unv;
 *       loc(f, j) = fsub(1, fmul(S[f][l], tilt[j-1])); a loc that comes out NaN (NaN or Inf samples inside len) counts as +inf.
 *       State 0 is always finite, so a best path always exists.
 * Transition:  0 -> 0 costs 0;  0 <-> j costs w_switch;  j' -> j costs fmul(w_jump, fabsf(fsub(lg[j-1], lg[j'-1]))).
 * Recurrence:  D[0][j] = loc(0, j);  D[f][j] = fadd(loc(f, j), min over j' of fadd(D[f-1][j'], trans(j', j))), the argmin taking the
 *       smallest j' on ties.  End: the smallest j among the minima of D[F_b - 1]; then the back pointers are followed.  The minimum
 *       of a set of floats does not depend on the order it is taken in, so numpy reproduces lag bit for bit given S.
 * Out:  lag i32 (B,Fmax): 0 for unvoiced, else the lag; peak f32 (B,Fmax,3) = (S[l-1], S[l], S[l+1]) copied from S, a neighbour
 *       outside [lmin, lmax] being S[l]; (0, 0, 0) for unvoiced; nccf f32 (B,Fmax,L) or NULL: S for f < F_b.  Nothing at or behind
 *       F_b is written in any output, F_b = 0 writes nothing.  audio and the outputs must not overlap.
 * Workspace: smtts_pitch_workspace_bytes(B, row_stride, hop, lmin, lmax) bytes, 256-byte aligned: the scores (also when nccf is
 *       given) and the back pointers, uint16 (B,Fmax,L+1).  What it holds before the call does not matter.
 * Two launches whatever B is (scores: one workgroup per row and 8 frames; path: one workgroup per row, the frames of a row are a
 *       chain); no atomics, nothing depends on scheduling: two calls on equal inputs return equal bits, and a row's results do not
 *       depend on its batch-mates.
 * Refused with 1 (the query: 0) and a message naming the entry, nothing enqueued: a NULL handle, audio, len, tab, lag, peak or ws; B
 *       outside [1, 1024]; row_stride outside [1, 2^24]; hop outside [16, 1024] or not a multiple of 4; win outside [32, 2048] or not
 *       a multiple of 4; lmin < 2, lmax <= lmin, lmax > 2048 or L > 1023; bias <= 0 or not finite; c_unv, w_jump or w_switch negative
 *       or not finite; ws_bytes below the query, or ws not 256-byte aligned. */
size_t smtts_pitch_workspace_bytes(smtts_handle h, int B, int64_t row_stride, int hop, int lmin, int lmax);
int smtts_pitch(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len /* DEVICE (B) */,
                const float* tab /* DEVICE f32 (2,L) */, int hop, int win, int lmin, int lmax, float bias, float c_unv, float w_jump,
                float w_switch, int32_t* lag /* (B,Fmax) */, float* peak /* (B,Fmax,3) */, float* nccf /* (B,Fmax,L) or NULL */,
                void* ws, size_t ws_bytes);

/* cond_encode runs the text encoder on a side stream owned by the engine, one per caller stream (fork / join with events; default
 * on: shortest latency for one batch at a time).  Callers that keep several batches in flight on their own streams should turn it
 * off (throughput tuning does): twice the streams cost more than the overlap buys (7.96 -> 9.59 ms per batch at three in flight). */
int smtts_set_dual_stream(smtts_handle h, int on);
/* Tuning mode: 0 = latency (default: one batch at a time finishes as early as possible: split-K on the small-M projections, deep
 * DMA rings, text encoder on the side stream), 1 = throughput (the caller keeps several independent batches in flight on its own
 * streams: unsplit GEMMs, no side stream, persistent codec kernels on three quarters of the CUs, so that kernels cost the fewest CU-microseconds and leave LDS for the
 * other streams).  Results differ between the modes only by fp32 summation order. */
int smtts_set_tuning(smtts_handle h, int mode);

/* per-kernel HIP-event timing on the launch stream (bench.py roofline): enable, run, then read a JSON array
 * [{"name","launches","ms","flops","bytes"}] of algorithmic work and measured time per kernel class */
int smtts_profile_enable(smtts_handle h, int on);   /* 0 off, 1 per kernel class, 2 + pipeline phase prefix, 3 + GEMM shapes */
int smtts_profile_report(smtts_handle h, char* buf, size_t cap);

/* ---- single-kernel test hooks (used by tests/ to check kernels in isolation) -------------------- */
/* C[M,N] = A[M,K] (f32, lda) * W[N,K]^T (f32 host-layout on device, split internally) + bias ; act as ACT_* */
/* microbenchmark of one GEMM launch configuration (epi: 0 store, 1 store+gelu, 2 swiglu, 3 tanh-gated residual) */
int smtts_bench_gemm(smtts_handle h, int M, int N, int K, int epi, int split, int cfg, int iters, int ver /* kernel generation 1 (fp32 A, register-staged) | 3 (gemm3) */,
                     float* avg_us);
/* hot-path kernel (gemm3: split-bf16 A and W via DMA ring): C[M,N] = act(A W^T + bias); A, W fp32 on device, split internally; K % 64 == 0 */
int smtts_test_gemm3(smtts_handle h, void* stream, const float* A, const float* W, const float* bias, int M, int N, int K,
                     int act, int split, int cfg, float* C);
/* one LN-fold step (the AdaLN / RMSNorm between two block GEMMs, see smtts_test_set_ln_fold) on its own:
 *   x[m] += row_mask[m] gate (A[m] Wp^T + bp)          (x [M,D] updated in place; masked rows keep x; gate / bp / row_mask may be null)
 *   y = LN(x; eps) (1 + scale) + shift   (rms = 0)   or   y = x rsqrt(mean x^2 + eps) scale   (rms = 1, shift unused)
 *   hid[M,F] = silu(y W1^T + b1) * (y W3^T + b3)       (fp32, decoded from the 16-bit operand image the chain writes)
 * fold = 1: the producer / consumer epilogues with the tables of fold_vectors; 0: the norm launches.  prec 1 bf16, 2 fp16,
 * 3 split-bf16 for every operand.  K % 64 == 0, D % 32 == 0 (fold: D % 64 == 0, and D == 960 with rms = 0), F % 32 == 0.
 * shift_out [M] (may be null): the producers' row shift as the consumer leaves it for the next producer (the mean of the updated
 * row, LayerNorm fold only; 0 otherwise) */
int smtts_test_ln_fold(smtts_handle h, void* stream, const float* A, const float* Wp, const float* bp, const float* gate,
                       const uint8_t* row_mask, const float* scale, const float* shift, const float* W1, const float* W3,
                       const float* b1, const float* b3, int M, int K, int D, int F, float eps, int rms, int prec, int fold,
                       float* x, float* hid, float* shift_out);
/* one codec stage of the finalized decoder (part 1) or encoder (part 2), through the same code as smtts_codec_decode / _encode and
 * a workspace planned for the smallest whole call that contains this stage geometry (so the same kernels run).
 *   what: 1 = the stem (stage must be 0), 2 = the resampling into `stage` (stage > 0), 4 = the stage's blocks (chain or one by one,
 *   as the product decides), 8 = final norm (if loaded) + head (stage must be the last); bits may be combined as a run in that order.
 *   x: device fp32, channels-last, unpadded (B, T_in, C_in): C_in = latent (decoder stem), 1 (encoder stem: T_in samples), the
 *   previous stage's C (resampling) or the stage's C; encoder resampling needs T_in % ratio == 0.
 *   out: (B, T_out, C_out) (decoder head: C_out = 1, the audio); out == NULL only reports T_out / C_out.
 * Allocates its own padded images and workspace (filled with NaN first: a kernel that reads what nobody wrote shows up) and
 * synchronises the stream.  Refuses a bad part / stage / `what` / C_in or B*T <= 0
 * with an error and no launch. */
int smtts_test_codec_stage(smtts_handle h, void* stream, int part, int stage, int what, const float* x, int B, int T_in, int C_in,
                           float* out, int* T_out, int* C_out);
/* one carry_frames launch (codec_stream.hip) on an image of the caller's: img f32 [B][8 + T][C], C a multiple of 4; the boundary's
 * [8][C] block lies `offset` bytes into slot slots[b] (DEVICE int64 (B), each slot once) of a pool with `slot_stride` bytes per slot; img,
 * state_pool, slot_stride and offset 16-byte aligned.  pad frame j <- block[j]; block[j] <- frame T - 8 + j of the row where that is
 * >= 0, block[j + T] otherwise.  This hook knows no pool size: negative indices are clamped to 0, others are the caller's to keep in range. */
int smtts_test_carry_frames(smtts_handle h, void* stream, float* img, int B, int T, int C, void* state_pool, int64_t slot_stride,
                            int64_t offset, const int64_t* slots);
/* DiT / condition-encoder stages through the code of smtts_denoise_step / smtts_sample / smtts_cond_encode.  net: 0 DiT, 1 style
 * encoder, 2 text encoder.  what (a run of the chain bits, in pipeline order):
 *   DiT:      1 modulation table from t[mod_rows] (otherwise `mod` [mod_rows][71040] is the table; either feeds the blocks), 2 embed
 *             (x = latents [B][S][64] -> residual), 4 blocks [l0, l1) (x = residual [B][S][960] unless 2 ran), 8 velocity head (x = the
 *             final AdaLN image [B][S][960] unless 4 ran; out = velocity [B][S][64]);
 *   encoders: 1 input (style: x = ref [B][S][64]; text: x = int64 ids [B][S]), 2 blocks [l0, l1) (x = residual [B][S][512] unless 1
 *             ran), 4 output projection (x = final norm image [B][S][512] unless 2 ran; out = ref_seq / phoneme memory [B][S][960]),
 *             8 cross K / V of the 12 DiT blocks (x = [B][S][960] unless 4 ran; k_out, v_out [12][B][8][S][120]).
 * path of the blocks: 0 the operator's choice (denoise_step's for the DiT), 1 LN-fold, 2 split-K + norm launches, 3 unsplit GEMM + norm
 * launch; a path the product never takes there (fold with M > 1024 or mod_rstride != 0, split-K with M > 1024) is refused.  mask: the
 * self / key mask [B][S]; k_ref .. ph_mask, R, P, rope: as smtts_denoise_step.  mod_row0 / mod_rstride (0 or 1): the modulation row
 * of utterance b is mod_row0 + b mod_rstride.  Outputs (each may be NULL): x_out residual after the last embed / input / block stage,
 * img_out the AdaLN / RMSNorm operand image the blocks leave for the next GEMM decoded to fp32 (fold: (x - shift) (1 + scale) of the
 * next block / x weight), shift_out [B][S] the fold's row shift (zeros off the fold), mod_out the modulation table.  The workspace
 * is planned as the operators plan it and filled with 0xff (NaN) first; twice != 0 runs everything a second time on it, as the
 * sampler's later steps find it.  Synchronises the stream; bad arguments are refused before any launch. */
int smtts_test_dit_stage(smtts_handle h, void* stream, int net, int what, int l0, int l1, int path, int twice, const void* x,
                         const uint8_t* mask, int B, int S, const float* t, const float* mod, int mod_rows, int mod_row0, int mod_rstride,
                         const float* k_ref, const float* v_ref, const uint8_t* ref_mask, int R, const float* k_text,
                         const float* v_text, const uint8_t* ph_mask, int P, const float* rope, float* x_out, float* img_out,
                         float* shift_out, float* out, float* k_out, float* v_out, float* mod_out);
/* Every launch of one scorer call, tapped.  net 0: smtts_asr_logprobs (out = logp (B, 4 N, 198)); net 1: smtts_sv_embed (out = emb
 * (B, 192)).  The hook calls the product's own launcher with a tap sink (null in every product call): behind each launch the whole
 * per-call buffer that launch wrote is copied, on the same stream, to the launch's slot of `taps`, before a later launch overwrites
 * it (the recogniser's residual is updated in place, the verifier reuses three buffers per block and lays the pooling logits over
 * them).  The workspace is this hook's own: the product's size function, filled with 0xff first, so that a launch which read what
 * nobody wrote leaves NaN in its tap; rows at and behind a row's length hold that NaN, they are nobody's to write.
 * Slots, one per launch in launch order, each the fp32 buffer named (T = 4 N):
 *   net 0 (44): 0 upsample (B, T, 64); for layer l = 0 .. 6 at 1 + 6 l: ffn1 (B, T, 64), qkv (B, T, 192: q times 0.5, k, v), attn
 *               (B, T, 64), proj (B, T, 64), conv (B, T, 64), ffn2 with the final LayerNorm (B, T, 64); 43 head = logp (B, T, 198)
 *   net 1 (23): 0 blocks.0 (B, N, 768); for block i = 0 .. 2 at 1 + 5 i: tdnn1 (B, N, 768), res2net (B, N, 768), tdnn2 (B, N, 768),
 *               se gate (B, 768), se apply + residual (B, N, 768); 16 mfa (B, N, 2304), 17 uniform [mean ; std] (B, 4608), 18 the
 *               attention's row constant (B, 192), 19 attention tanh (B, N, 192), 20 pooling logits (B, N, 2304), 21 pooled behind
 *               asp_bn (B, 4608), 22 fc = emb (B, 192)
 * smtts_test_scorer_tap_bytes: the size of the tap buffer (0 when refused); off, when not NULL, holds cap >= 44 (net 0) / 23 (net 1)
 * entries and receives the byte offset of every slot (multiples of 256, in launch order).
 * smtts_test_scorer_taps refuses what the entry itself refuses (no such part, B, N, NULL or misaligned x / n_len / out), a NULL or
 * not 256-byte aligned `taps` and tap_bytes under that size, each with an error and nothing enqueued.  Synchronises the stream. */
size_t smtts_test_scorer_tap_bytes(smtts_handle h, int net, int B, int N, size_t* off, int cap);
int smtts_test_scorer_taps(smtts_handle h, void* stream, int net, const float* x, const int32_t* n_len, int B, int N, float* out,
                           void* taps, size_t tap_bytes);
/* codec blocks: 1 (default) = fused mixer and fused FFN kernels (C <= 256), 0 = separate norm / conv / two-GEMM path */
int smtts_test_set_fused_ffn(smtts_handle h, int on);
/* fused sampler: 1 (default) = the AdaLN between two DiT block GEMMs folded into their epilogues (reference dit.py:19-25,197-212
 * restated as rstd (x (1 + scale) W^T - mu W (1 + scale)) + W shift + b), 0 = split-K reduce + norm (latency) / ln_modulate (throughput) launches.
 * Workspace sizes depend on it: query them after the call. */
int smtts_test_set_ln_fold(smtts_handle h, int on);
int smtts_test_gemm(smtts_handle h, void* stream, const float* A, int lda, const float* W, const float* bias, int M,
                    int N, int K, int act, int split, int cfg, float* C, int ldc);
int smtts_test_swiglu(smtts_handle h, void* stream, const float* A, const float* W1, const float* W3, const float* b1,
                      const float* b3, int M, int F, int K, int split, float* out);
int smtts_test_attention(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                         const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                         const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                         const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* out);

/* the product's attention path in isolation: stand-alone producers (qkv_pack + cross_pack) write the operand images, then the DMA + MFMA
 * kernel (attention_img.hip) at the site-7 operand precision; same contract as smtts_test_attention (the fp32 VALU reference) */
int smtts_test_attention_mfma(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                              const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                              const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                              const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* out);
/* the text-attention tap (smtts_sample_align) in isolation, on the images smtts_test_attention_mfma builds from the same inputs:
 * mass f32 (B,N,P) = the mean over all H heads of each frame's softmax probability on each text key.  P > 0. */
int smtts_test_attn_text_mass(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                              const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                              const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                              const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* mass);
/* engine-wide A/B switch: non-zero (default) = operand images written by the QKVG GEMM epilogue + the DMA / MFMA attention kernel;
 * 0 = fp32 projection + in-place qk_prep + the fp32 VALU reference kernel */
int smtts_test_set_attention_mfma(smtts_handle h, int mode);

#ifdef __cplusplus
}
#endif
#endif
