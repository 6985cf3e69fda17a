// extern "C" surface of libsmalltts_hip.so — see include/smalltts_hip.h for the contract.
#include "../../include/smalltts_hip.h"

#include <cstdint>
#include <cstring>
#include <string>

#include "capi_handle.hpp"

thread_local std::string g_create_err;

extern "C" {

const char* smtts_version(void) { return "smalltts-hip 0.5 (gfx950)"; }
int smtts_abi_version(void) { return SMTTS_ABI_VERSION; }

int smtts_create(int device_id, smtts_handle* out) {
    if (!out) return 1;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device_id < 0 || device_id >= n) {
        g_create_err = e != hipSuccess ? std::string("hipGetDeviceCount: ") + hipGetErrorString(e)
                                       : "device id out of range (have " + std::to_string(n) + " GPUs)";
        return 1;
    }
    e = hipSetDevice(device_id);
    if (e != hipSuccess) { g_create_err = hipGetErrorString(e); return 1; }
    *out = new smtts_engine(device_id);
    return 0;
}
int smtts_destroy(smtts_handle h) { delete h; return 0; }  // NULL is a no-op, like free()
const char* smtts_last_error(smtts_handle h) { return h ? E.last_error().c_str() : g_create_err.c_str(); }

int smtts_set_tensor(smtts_handle h, const char* name, const float* data, const int64_t* shape, int ndim, int on_dev) { NULLCHK;
    long sh[8];
    if (ndim > 8) return E.fail("set_tensor: ndim > 8");
    for (int i = 0; i < ndim; ++i) sh[i] = (long)shape[i];
    return E.set_tensor(name, data, sh, ndim, on_dev != 0);
}
int smtts_synth_tensor(smtts_handle h, const char* name, const int64_t* shape, int ndim, uint64_t key, float mean,
                       float half_range) { NULLCHK;
    long sh[8];
    if (ndim > 8) return E.fail("synth_tensor: ndim > 8");
    for (int i = 0; i < ndim; ++i) sh[i] = (long)shape[i];
    return E.synth_tensor(name, sh, ndim, key, mean, half_range);
}
int smtts_get_tensor(smtts_handle h, const char* name, float* host_out, int64_t numel) { NULLCHK;
    return E.get_tensor(name, host_out, (long)numel);
}
int smtts_set_codec_spec(smtts_handle h, int latent_dim, int n_filters, int kernel, int ffn_mult, float eps,
                         const int* ratios, int n_ratios, const int* depths) { NULLCHK;
    CodecSpecC s;
    if (n_ratios < 1 || n_ratios > 7) return E.fail("codec spec: 1..7 ratios supported");
    s.latent_dim = latent_dim; s.n_filters = n_filters; s.kernel = kernel; s.ffn_mult = ffn_mult; s.eps = eps;
    s.n_ratios = n_ratios;
    for (int i = 0; i < 8; ++i) s.ratios[i] = i < n_ratios ? ratios[i] : 0;
    for (int i = 0; i < 9; ++i) s.depths[i] = i <= n_ratios ? depths[i] : 0;
    return E.set_codec_spec(s);
}
int smtts_finalize(smtts_handle h) { NULLCHK; return E.finalize(); }
int smtts_set_precision(smtts_handle h, int preset) { NULLCHK;
    if (preset < 1 || preset > 3) return E.fail("precision preset must be 1 (bf16), 2 (f16 mixed) or 3 (split-bf16)");
    E.set_precision(preset);
    return 0;
}
int smtts_get_precision(smtts_handle h) { NULLCHK; return E.precision(); }
int smtts_default_precision(void) { return kDefaultPrecision; }
int smtts_set_site_precision(smtts_handle h, int site, int prec) { NULLCHK; return E.set_site_precision(site, prec); }
int smtts_get_saturations(smtts_handle h, uint32_t* counts, int n_sites, int reset) { NULLCHK;
    if (!counts || n_sites < 0) return E.fail("get_saturations: bad arguments");
    return E.get_saturations(counts, n_sites, reset != 0);
}
int smtts_peek_saturations(smtts_handle h, uint32_t* counts, int n_sites) { NULLCHK;
    if (!counts || n_sites < 0) return E.fail("peek_saturations: bad arguments");
    return E.peek_saturations(counts, n_sites);
}
const char* smtts_range_report(smtts_handle h) {
    if (!h) { g_create_err = std::string(__func__) + ": null handle"; return ""; }
    return E.range_report().c_str();
}
float smtts_range_worst_bound(smtts_handle h) { NULLCHK0; return E.range_worst(); }
int smtts_has_part(smtts_handle h, int part) { NULLCHK0;
    return part == 0 ? E.has_dit() : part == 1 ? E.has_decoder() : part == 2 ? E.has_encoder() : part == 3 ? E.has_asr() : part == 4 ? E.has_sv() : 0;
}

size_t smtts_cond_workspace_bytes(smtts_handle h, int B, int R, int P) { NULLCHK0; return E.cond_ws_bytes(B, R, P); }
int smtts_cond_encode(smtts_handle h, void* stream, const float* ref, const int64_t* ref_len, const int64_t* phonemes,
                      const uint8_t* ph_mask, int B, int R, int P, float* k_ref, float* v_ref, uint8_t* ref_mask,
                      float* k_text, float* v_text, void* ws, size_t ws_bytes, float* ref_seq_out, float* mem_out) { NULLCHK;
    return E.cond_encode(ST(stream), ref, ref_len, phonemes, ph_mask, B, R, P, k_ref, v_ref, ref_mask, k_text, v_text, ws,
                         ws_bytes, ref_seq_out, mem_out);
}

size_t smtts_denoise_workspace_bytes(smtts_handle h, int B, int N, int R, int P) { NULLCHK0; return E.denoise_ws_bytes(B, N, R, P, B); }
int smtts_denoise_step(smtts_handle h, void* stream, const float* x_t, const uint8_t* mask, const float* t,
                       const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
                       const float* v_text, const uint8_t* ph_mask, const float* rope, int B, int N, int R, int P,
                       float* velocity, void* ws, size_t ws_bytes) { NULLCHK;
    return E.denoise_step(ST(stream), x_t, mask, t, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask, rope, B, N, R, P,
                          velocity, ws, ws_bytes);
}

size_t smtts_sample_workspace_bytes(smtts_handle h, int B, int N, int R, int P, int n_steps, int cfg) { NULLCHK0;
    return E.sample_ws_bytes(B, N, R, P, n_steps, cfg);
}
int smtts_sample(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                 const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                 const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                 const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes) { NULLCHK;
    return E.sample(ST(stream), mode, n_steps, cfg, s_text, s_spk, mask, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask,
                    B, N, R, P, noise, seed, x_out, steps_out, ws, ws_bytes);
}

int smtts_sample_align(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                       const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                       const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                       const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes,
                       const uint8_t* tap_steps, uint32_t tap_layers, uint32_t tap_heads, float* text_mass) { NULLCHK;
    return E.sample_align(ST(stream), mode, n_steps, cfg, s_text, s_spk, mask, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask,
                          B, N, R, P, noise, seed, x_out, steps_out, ws, ws_bytes, tap_steps, tap_layers, tap_heads, text_mass);
}
int smtts_sample_pinned(smtts_handle h, void* stream, int mode, int n_steps, int cfg, float s_text, float s_spk,
                        const uint8_t* mask, const float* k_ref, const float* v_ref, const uint8_t* ref_mask,
                        const float* k_text, const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P,
                        const float* noise, uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes,
                        const uint8_t* tap_steps, uint32_t tap_layers, uint32_t tap_heads, float* text_mass, const float* x_pin,
                        const uint8_t* pin, int start_step) { NULLCHK;
    return E.sample_pinned(ST(stream), mode, n_steps, cfg, s_text, s_spk, mask, k_ref, v_ref, ref_mask, k_text, v_text, ph_mask,
                           B, N, R, P, noise, seed, x_out, steps_out, ws, ws_bytes, tap_steps, tap_layers, tap_heads, text_mass, x_pin,
                           pin, start_step);
}
int smtts_align_path(smtts_handle h, void* stream, const float* mass, int B, int N, int P, const int32_t* n_len, const int32_t* p0,
                     const int32_t* p1, int32_t* spans, float* score) { NULLCHK;
    if (B <= 0 || !mass || !n_len || !p0 || !p1 || !spans || !score) return E.fail("align_path: bad arguments");
    if (N < 1 || P < 1 || N > 225 || P > 198) return E.fail("align_path: N must be in [1, 225] and P in [1, 198] (the back-pointers of a row live in LDS)");
    hipError_t e = launch_align_path(mass, B, N, P, n_len, p0, p1, spans, score, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "align_path");
}

int smtts_take_scores(smtts_handle h, void* stream, const float* mass, const int32_t* spans, const float* path_score, const int32_t* n_len,
                      const int32_t* p0, const int32_t* p1, int B, int N, int P, float tau_tok, float tau_frm, float w0, float w1, float w2,
                      float w3, int32_t* feat, float* total) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_take_scores: B must be in [1, 65536]");
    if (N < 1 || P < 1 || N > 225 || P > 198) return E.fail("smtts_take_scores: N must be in [1, 225] and P in [1, 198] (the range of smtts_align_path)");
    if (!mass || !spans || !path_score || !n_len || !p0 || !p1 || !feat || !total) return E.fail("smtts_take_scores: a required pointer is NULL");
    if (!(w0 >= 0.f) || !(w1 >= 0.f) || !(w2 >= 0.f) || !(w3 >= 0.f)) return E.fail("smtts_take_scores: the weights must be >= 0 (and not NaN)");
    if (tau_tok != tau_tok || tau_frm != tau_frm) return E.fail("smtts_take_scores: the thresholds must not be NaN");
    hipError_t e = launch_take_scores(mass, spans, path_score, n_len, p0, p1, B, N, P, tau_tok, tau_frm, w0, w1, w2, w3, feat, total, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "take_scores");
}
int smtts_take_select(smtts_handle h, void* stream, const float* total, int G, int K, int N, int P, const float* x, const int32_t* n_len,
                      const int32_t* spans, const float* mass, float* x_win, int32_t* n_win, int32_t* spans_win, float* mass_win,
                      int32_t* winner) { NULLCHK;
    if (G < 1 || G > 65535) return E.fail("smtts_take_select: G must be in [1, 65535]");
    if (K < 1 || K > 16) return E.fail("smtts_take_select: K must be in [1, 16]");
    if (N < 1 || P < 1 || N > 225 || P > 198) return E.fail("smtts_take_select: N must be in [1, 225] and P in [1, 198] (the range of smtts_align_path)");
    if (!total || !x || !n_len || !x_win || !n_win || !winner) return E.fail("smtts_take_select: a required pointer is NULL");
    if ((spans != nullptr) != (spans_win != nullptr) || (mass != nullptr) != (mass_win != nullptr))
        return E.fail("smtts_take_select: spans / spans_win and mass / mass_win are given or NULL together");
    hipError_t e = launch_take_select(total, G, K, N, P, x, n_len, spans, mass, x_win, n_win, spans_win, mass_win, winner, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "take_select");
}

int smtts_repair_plan(smtts_handle h, void* stream, const float* mass, const int32_t* spans, const int32_t* n_len, const int32_t* p0,
                      const int32_t* p1, const uint8_t* keep, int B, int N, int P, float tau_tok, int max_span, int margin, uint8_t* pin,
                      int32_t* counts) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_repair_plan: B must be in [1, 65536]");
    if (N < 1 || P < 1 || N > 225 || P > 198) return E.fail("smtts_repair_plan: N must be in [1, 225] and P in [1, 198] (the range of smtts_align_path)");
    if (!mass || !spans || !n_len || !p0 || !p1 || !pin || !counts) return E.fail("smtts_repair_plan: a required pointer is NULL");
    if (max_span < 1 || max_span > 225) return E.fail("smtts_repair_plan: max_span must be in [1, 225]");
    if (margin < 0 || margin > 32) return E.fail("smtts_repair_plan: margin must be in [0, 32]");
    if (tau_tok != tau_tok) return E.fail("smtts_repair_plan: the threshold must not be NaN");
    hipError_t e = launch_repair_plan(mass, spans, n_len, p0, p1, keep, B, N, P, tau_tok, max_span, margin, pin, counts, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "repair_plan");
}
int smtts_repair_keep(smtts_handle h, void* stream, int G, int N, int P, const float* total_cur, const float* total_new,
                      const int32_t* counts, const int32_t* feat_cur, const int32_t* feat_new, float* x_cur, const float* x_new,
                      int32_t* spans_cur, const int32_t* spans_new, float* mass_cur, const float* mass_new, float* total_out,
                      int32_t* feat_out, int32_t* kept) { NULLCHK;
    if (G < 1 || G > 65535) return E.fail("smtts_repair_keep: G must be in [1, 65535]");
    if (N < 1 || P < 1 || N > 225 || P > 198) return E.fail("smtts_repair_keep: N must be in [1, 225] and P in [1, 198] (the range of smtts_align_path)");
    if (!total_cur || !total_new || !counts || !feat_cur || !feat_new || !x_cur || !x_new || !total_out || !feat_out || !kept)
        return E.fail("smtts_repair_keep: a required pointer is NULL");
    if ((spans_cur != nullptr) != (spans_new != nullptr) || (mass_cur != nullptr) != (mass_new != nullptr))
        return E.fail("smtts_repair_keep: spans_cur / spans_new and mass_cur / mass_new are given or NULL together");
    hipError_t e = launch_repair_keep(G, N, P, total_cur, total_new, counts, feat_cur, feat_new, x_cur, x_new, spans_cur, spans_new, mass_cur,
                                      mass_new, total_out, feat_out, kept, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "repair_keep");
}

size_t smtts_asr_workspace_bytes(smtts_handle h, int B, int N) { NULLCHK0; return E.asr_workspace_bytes(B, N); }
int smtts_asr_logprobs(smtts_handle h, void* stream, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes,
                       float* logp) { NULLCHK;
    return E.asr_logprobs(ST(stream), x, n_len, B, N, ws, ws_bytes, logp);
}
int smtts_ctc_score(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                    const int32_t* p1, int B, int T, int P, int C, float* nll) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_ctc_score: B must be in [1, 65536]");
    if (T < 1 || T > 65536 || P < 1 || P > 198 || C < 2 || C > 256)
        return E.fail("smtts_ctc_score: T must be in [1, 65536], P in [1, 198] and C in [2, 256] (a row's states and emission ring live in LDS)");
    if (!logp || !t_len || !tokens || !p0 || !p1 || !nll) return E.fail("smtts_ctc_score: a required pointer is NULL");
    hipError_t e = launch_ctc_score(logp, t_len, tokens, p0, p1, B, T, P, C, nll, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "ctc_score");
}
int smtts_ctc_greedy(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, int B, int T, int C, int32_t* ids,
                     int32_t* n_ids) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_ctc_greedy: B must be in [1, 65536]");
    if (T < 1 || T > 4096 || C < 1 || C > 65536) return E.fail("smtts_ctc_greedy: T must be in [1, 4096] (a row's classes live in LDS) and C in [1, 65536]");
    if (!logp || !t_len || !ids || !n_ids) return E.fail("smtts_ctc_greedy: a required pointer is NULL");
    hipError_t e = launch_ctc_greedy(logp, t_len, B, T, C, ids, n_ids, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "ctc_greedy");
}
int smtts_ctc_align(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                    const int32_t* p1, int B, int T, int P, int C, int32_t* spans, float* tok_logp, int32_t* frame_tok, float* score) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_ctc_align: B must be in [1, 65536]");
    if (T < 1 || T > 1024 || P < 1 || P > 198 || C < 2 || C > 256)
        return E.fail("smtts_ctc_align: T must be in [1, 1024], P in [1, 198] and C in [2, 256] (a row's states, moves and emission ring live in LDS)");
    if (!logp || !t_len || !tokens || !p0 || !p1 || !spans || !tok_logp || !score) return E.fail("smtts_ctc_align: a required pointer is NULL");
    hipError_t e = launch_ctc_align(logp, t_len, tokens, p0, p1, B, T, P, C, spans, tok_logp, frame_tok, score, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "ctc_align");
}

size_t smtts_ctc_align_long_workspace_bytes(smtts_handle h, int B, int T, int P) { NULLCHK0;
    if (B < 1 || B > 64) return 0;
    return ctc_align_long_ws_bytes(B, T, P);
}
int smtts_ctc_align_long(smtts_handle h, void* stream, const float* logp, const int32_t* t_len, const int32_t* tokens, const int32_t* p0,
                         const int32_t* p1, int B, int T, int P, int C, int32_t* spans, float* tok_logp, int32_t* frame_tok, float* score,
                         void* ws, size_t ws_bytes) { NULLCHK;
    if (B < 1 || B > 64) return E.fail("smtts_ctc_align_long: B must be in [1, 64]");
    if (T < 1 || T > 65536 || P < 1 || P > 16383 || C < 2 || C > 256)
        return E.fail("smtts_ctc_align_long: T must be in [1, 65536], P in [1, 16383] and C in [2, 256] (32 extended states per thread of one workgroup)");
    if (!logp || !t_len || !tokens || !p0 || !p1 || !spans || !tok_logp || !score) return E.fail("smtts_ctc_align_long: a required pointer is NULL");
    if (!ws || ((uintptr_t)ws & 255)) return E.fail("smtts_ctc_align_long: the workspace must be 256-byte aligned");
    if (ws_bytes < ctc_align_long_ws_bytes(B, T, P))
        return E.fail("smtts_ctc_align_long: the workspace is smaller than smtts_ctc_align_long_workspace_bytes(h, B, T, P)");
    hipError_t e = launch_ctc_align_long(logp, t_len, tokens, p0, p1, B, T, P, C, spans, tok_logp, frame_tok, score, ws, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "ctc_align_long");
}

size_t smtts_sv_workspace_bytes(smtts_handle h, int B, int N) { NULLCHK0; return E.sv_workspace_bytes(B, N); }
int smtts_sv_embed(smtts_handle h, void* stream, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes,
                   float* emb) { NULLCHK;
    return E.sv_embed(ST(stream), x, n_len, B, N, ws, ws_bytes, emb);
}
int smtts_sv_cosine(smtts_handle h, void* stream, const float* emb, const float* ref, int B, int K, int D, float* cos) { NULLCHK;
    if (B < 1 || B > 65536) return E.fail("smtts_sv_cosine: B must be in [1, 65536]");
    if (K < 1 || K > 16 || B % K || D < 1 || D > 1024)
        return E.fail("smtts_sv_cosine: K must be in [1, 16] and divide B, D must be in [1, 1024]");
    if (!emb || !ref || !cos) return E.fail("smtts_sv_cosine: a required pointer is NULL");
    if (((uintptr_t)emb | (uintptr_t)ref | (uintptr_t)cos) & 3) return E.fail("smtts_sv_cosine: emb, ref and cos must be 4-byte aligned");
    hipError_t e = launch_sv_cosine(emb, ref, B, K, D, cos, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "sv_cosine");
}

int smtts_codec_hop(smtts_handle h) { NULLCHK0; return E.codec_spec().hop(); }
size_t smtts_decode_workspace_bytes(smtts_handle h, int B, int T) { NULLCHK0; return E.decode_ws_bytes(B, T); }
int smtts_codec_decode(smtts_handle h, void* stream, const float* latents, int B, int T, float* audio, void* ws,
                       size_t ws_bytes) { NULLCHK;
    return E.codec_decode(ST(stream), latents, B, T, audio, ws, ws_bytes);
}
size_t smtts_decode_state_bytes(smtts_handle h) { NULLCHK0;
    if (!E.has_decoder()) { E.fail("smtts_decode_state_bytes: decoder weights not finalized"); return 0; }
    return E.decode_state_layout().bytes;
}
size_t smtts_decode_stream_workspace_bytes(smtts_handle h, int B, int T) { NULLCHK0;
    if (B < 1 || T < 1) { E.fail("smtts_decode_stream_workspace_bytes: B and T must be positive"); return 0; }
    return E.decode_ws_bytes(B, T);
}
int smtts_codec_decode_stream(smtts_handle h, void* stream, const float* latents, int B, int T, void* state_pool, int64_t n_slots,
                              const int64_t* slots, float* audio, void* ws, size_t ws_bytes) { NULLCHK;
    return E.codec_decode_stream(ST(stream), latents, B, T, state_pool, n_slots, slots, audio, ws, ws_bytes);
}
int smtts_test_carry_frames(smtts_handle h, void* stream, float* img, int B, int T, int C, void* state_pool, int64_t slot_stride,
                            int64_t offset, const int64_t* slots) { NULLCHK;
    if (B < 1 || T < 1 || C < 4 || C % 4) return E.fail("smtts_test_carry_frames: B, T >= 1 and C a positive multiple of 4");
    if (!img || !state_pool || !slots) return E.fail("smtts_test_carry_frames: a required pointer is NULL");
    if (offset < 0 || slot_stride < offset + 32 * (int64_t)C) return E.fail("smtts_test_carry_frames: the [8][C] block does not fit the slot");
    if (((uintptr_t)img | (uintptr_t)state_pool | (uintptr_t)slot_stride | (uintptr_t)offset) & 15)
        return E.fail("smtts_test_carry_frames: img, state_pool, slot_stride and offset must be 16-byte aligned");
    hipError_t e = launch_carry_frames(img, B, T, C, state_pool, (long)slot_stride, (long)offset, INT64_MAX, slots, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "carry_frames");
}
size_t smtts_encode_workspace_bytes(smtts_handle h, int B, int S) { NULLCHK0; return E.encode_ws_bytes(B, S); }
int smtts_codec_encode(smtts_handle h, void* stream, const float* audio, int B, int S, float* latents, void* ws,
                       size_t ws_bytes) { NULLCHK;
    return E.codec_encode(ST(stream), audio, B, S, latents, ws, ws_bytes);
}

int smtts_randn(smtts_handle h, void* stream, float* out, int64_t n, uint64_t seed, uint64_t stream_id) { NULLCHK;
    hipError_t e = launch_randn(out, (long)n, seed, stream_id, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "randn");
}

void smtts_alpha_sigma(float t, float* alpha, float* sigma) { alpha_sigma_host(t, *alpha, *sigma); }

int smtts_resample_poly(smtts_handle h, void* stream, const float* x, int channels, int64_t n_in, const float* bank, int up,
                        int down, int klen, int width, float* y, int64_t n_out) { NULLCHK;
    if (up <= 0 || down <= 0 || klen <= 0 || channels <= 0) return E.fail("resample_poly: bad arguments");
    hipError_t e = launch_resample_poly(x, n_in, bank, up, down, klen, width, y, n_out, channels, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "resample_poly");
}
int smtts_pcm16(smtts_handle h, void* stream, const float* x, int64_t n, int16_t* y) { NULLCHK;
    hipError_t e = launch_pcm16(x, y, n, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "pcm16");
}
int smtts_voice_expand(smtts_handle h, void* stream, const int64_t* table, int B, int Rmax, float* k_ref, float* v_ref,
                       uint8_t* ref_mask) { NULLCHK;
    if (B <= 0 || Rmax <= 0 || !table || !k_ref || !v_ref || !ref_mask) return E.fail("voice_expand: bad arguments");
    if ((((uintptr_t)k_ref | (uintptr_t)v_ref) & 15) != 0) return E.fail("voice_expand: k_ref / v_ref must be 16-byte aligned");
    hipError_t e = launch_voice_expand(table, k_ref, v_ref, ref_mask, B, Rmax, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "voice_expand");
}
int smtts_randn_rows(smtts_handle h, void* stream, float* out, const uint64_t* seeds, const int64_t* n, int n_steps, int B,
                     int Nmax) { NULLCHK;
    if (n_steps <= 0 || B <= 0 || Nmax <= 0 || !out || !seeds || !n) return E.fail("randn_rows: bad arguments");
    if (((uintptr_t)out & 15) != 0) return E.fail("randn_rows: out must be 16-byte aligned");
    hipError_t e = launch_randn_rows(out, seeds, n, n_steps, B, Nmax, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "randn_rows");
}
int smtts_stitch(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, const int64_t* off,
                 const float* fade, int F, void* out, int64_t out_n, int pcm16) { NULLCHK;
    if (B <= 0 || row_stride <= 0 || out_n <= 0 || F < 0 || !audio || !len || !off || !out || (F > 0 && !fade))
        return E.fail("stitch: bad arguments");
    hipError_t e = pcm16 ? launch_stitch_pcm16(audio, (long)row_stride, len, off, fade, F, static_cast<int16_t*>(out), (long)out_n, B,
                                               (long)row_stride, ST(stream))
                         : launch_stitch(audio, (long)row_stride, len, off, fade, F, static_cast<float*>(out), (long)out_n, B,
                                         (long)row_stride, ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "stitch");
}
int smtts_endpoints(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* len, int W, float rel_pow,
                    float floor_pow, int min_run, int lead, int tail, float target_rms, float peak_limit, float max_gain, float* e,
                    float* pk, int64_t* seg, float* gain) { NULLCHK;
    if (B <= 0 || row_stride <= 0 || !audio || !len || !e || !pk || !seg || !gain) return E.fail("endpoints: bad arguments");
    if (W < 16 || W > 4096 || (W & 3) != 0) return E.fail("endpoints: W must be a multiple of 4 in [16, 4096]");
    if (min_run < 1 || min_run > 16) return E.fail("endpoints: min_run must be in [1, 16]");
    if (lead < 0 || tail < 0) return E.fail("endpoints: lead and tail must not be negative");
    if (!(rel_pow >= 0.f) || !(floor_pow >= 0.f) || !(target_rms >= 0.f) || !(peak_limit > 0.f) || !(max_gain > 0.f))
        return E.fail("endpoints: rel_pow, floor_pow, target_rms must be >= 0 and peak_limit, max_gain > 0");
    hipError_t err = launch_endpoints(audio, (long)row_stride, len, W, rel_pow, floor_pow, min_run, lead, tail, target_rms, peak_limit,
                                      max_gain, e, pk, seg, gain, B, ST(stream));
    return err == hipSuccess ? 0 : E.fail_hip(err, "endpoints");
}
int smtts_stitch_seg(smtts_handle h, void* stream, const float* audio, int B, int64_t row_stride, const int64_t* seg, const float* gain,
                     const int64_t* off, const float* fade, int F, void* out, int64_t out_n, int pcm16) { NULLCHK;
    if (B <= 0 || row_stride <= 0 || out_n <= 0 || F < 0 || !audio || !seg || !off || !out || (F > 0 && !fade))
        return E.fail("stitch_seg: bad arguments");
    hipError_t e = launch_stitch_seg(audio, (long)row_stride, seg, gain, off, fade, F, out, (long)out_n, pcm16, B, (long)row_stride,
                                     ST(stream));
    return e == hipSuccess ? 0 : E.fail_hip(e, "stitch_seg");
}
int smtts_set_dual_stream(smtts_handle h, int on) { NULLCHK; E.set_dual_stream(on != 0); return 0; }
int smtts_set_tuning(smtts_handle h, int mode) { NULLCHK;
    if (mode != 0 && mode != 1) return E.fail("tuning mode must be 0 (latency) or 1 (throughput)");
    E.set_tuning(mode);
    return 0;
}
int smtts_profile_enable(smtts_handle h, int on) { NULLCHK; E.profile_enable(on); return 0; }
int smtts_profile_report(smtts_handle h, char* buf, size_t cap) { NULLCHK;
    std::string r = E.profile_report();
    if (r.size() + 1 > cap) return E.fail("profile_report: buffer too small");
    memcpy(buf, r.c_str(), r.size() + 1);
    return 0;
}

int smtts_bench_gemm(smtts_handle h, int M, int N, int K, int epi, int split, int cfg, int iters, int ver, float* avg_us) { NULLCHK;
    return E.bench_gemm(M, N, K, epi, split, cfg, iters, ver, avg_us);
}
int smtts_test_gemm3(smtts_handle h, void* stream, const float* A, const float* W, const float* bias, int M, int N, int K,
                     int act, int split, int cfg, float* C) { NULLCHK;
    return E.test_gemm3(ST(stream), A, W, bias, M, N, K, act, split, cfg, C);
}
int smtts_test_ln_fold(smtts_handle h, void* stream, const float* A, const float* Wp, const float* bp, const float* gate,
                       const uint8_t* row_mask, const float* scale, const float* shift, const float* W1, const float* W3,
                       const float* b1, const float* b3, int M, int K, int D, int F, float eps, int rms, int prec, int fold,
                       float* x, float* hid, float* shift_out) { NULLCHK;
    return E.test_ln_fold(ST(stream), A, Wp, bp, gate, row_mask, scale, shift, W1, W3, b1, b3, M, K, D, F, eps, rms, prec, fold, x, hid,
                          shift_out);
}
int smtts_test_codec_stage(smtts_handle h, void* stream, int part, int stage, int what, const float* x, int B, int T_in, int C_in,
                           float* out, int* T_out, int* C_out) { NULLCHK;
    return E.test_codec_stage(ST(stream), part, stage, what, x, B, T_in, C_in, out, T_out, C_out);
}
int smtts_test_dit_stage(smtts_handle h, void* stream, int net, int what, int l0, int l1, int path, int twice, const void* x,
                         const uint8_t* mask, int B, int S, const float* t, const float* mod, int mod_rows, int mod_row0, int mod_rstride,
                         const float* k_ref, const float* v_ref, const uint8_t* ref_mask, int R, const float* k_text,
                         const float* v_text, const uint8_t* ph_mask, int P, const float* rope, float* x_out, float* img_out,
                         float* shift_out, float* out, float* k_out, float* v_out, float* mod_out) { NULLCHK;
    return E.test_dit_stage(ST(stream), net, what, l0, l1, path, twice, x, mask, B, S, t, mod, mod_rows, mod_row0, mod_rstride, k_ref,
                            v_ref, ref_mask, R, k_text, v_text, ph_mask, P, rope, x_out, img_out, shift_out, out, k_out, v_out, mod_out);
}
size_t smtts_test_scorer_tap_bytes(smtts_handle h, int net, int B, int N, size_t* off, int cap) { NULLCHK0;
    return E.test_scorer_tap_bytes(net, B, N, off, cap);
}
int smtts_test_scorer_taps(smtts_handle h, void* stream, int net, const float* x, const int32_t* n_len, int B, int N, float* out,
                           void* taps, size_t tap_bytes) { NULLCHK;
    return E.test_scorer_taps(ST(stream), net, x, n_len, B, N, out, taps, tap_bytes);
}
int smtts_test_set_fused_ffn(smtts_handle h, int on) { NULLCHK; E.set_fused_ffn(on != 0); return 0; }
int smtts_test_set_ln_fold(smtts_handle h, int on) { NULLCHK; E.set_ln_fold(on != 0); return 0; }
int smtts_test_set_attention_mfma(smtts_handle h, int mode) { NULLCHK;   // 0: fp32 projection + qk_prep + the fp32 VALU reference kernel; else (default): producer-written operand images + the DMA / MFMA kernel
    E.set_attn_img(mode != 0);
    return 0;
}

// ---- test hooks -------------------------------------------------------------------------------
int smtts_test_gemm(smtts_handle h, void* stream, const float* A, int lda, const float* W, const float* bias, int M,
                    int N, int K, int act, int split, int cfg, float* C, int ldc) { NULLCHK;
    return E.test_gemm(ST(stream), A, lda, W, bias, M, N, K, act, split, cfg, C, ldc);
}
int smtts_test_swiglu(smtts_handle h, void* stream, const float* A, const float* W1, const float* W3, const float* b1,
                      const float* b3, int M, int F, int K, int split, float* out) { NULLCHK;
    return E.test_swiglu(ST(stream), A, W1, W3, b1, b3, M, F, K, split, out);
}
int smtts_test_attention(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                         const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                         const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                         const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* out) { NULLCHK;
#ifndef SMTTS_TEST_KERNELS
    return E.fail("smtts_test_attention: the fp32 VALU reference attention is not part of this build (make TEST_KERNELS=1)");
#else
    AttnArgs a{};
    const int D = H * dh;
    a.q = qkvg; a.k = qkvg + D; a.v = qkvg + 2 * D; a.gate = qkvg + 3 * D;
    a.bs = (long)N * 4 * D; a.rs = 4 * D;
    float *rc = nullptr, *rs = nullptr;
    const int nr = N * rot_dim;
    if (hipMalloc(&rc, (size_t)nr * 4) != hipSuccess || hipMalloc(&rs, (size_t)nr * 4) != hipSuccess)
        return E.fail("test_attention: alloc failed");
    (void)launch_rope_cossin(rope, rc, rs, nr, ST(stream));
    a.qw = qw; a.kw = kw; a.eps = eps; a.rope_cos = rc; a.rope_sin = rs; a.rot_dim = rot_dim;
    a.k_ref = R > 0 ? k_ref : nullptr; a.v_ref = v_ref; a.R = R;
    a.k_text = P > 0 ? k_text : nullptr; a.v_text = v_text; a.P = P;
    a.mask_self = mask_self; a.mask_ref = mask_ref; a.mask_text = mask_text;
    a.out = out; a.obs = (long)N * D; a.ors = D;
    a.B = B; a.N = N; a.H = H; a.dh = dh;
    hipError_t e = launch_attention(a, ST(stream));
    (void)hipStreamSynchronize(ST(stream));
    (void)hipFree(rc);
    (void)hipFree(rs);
    return e == hipSuccess ? 0 : E.fail_hip(e, "attention");
#endif
}

}  // extern "C"

// the product's attention path on stand-alone producers: out != null runs the DMA + MFMA kernel, mass != null the text-attention tap
// (all heads, mean) on the very same images
static int attn_img_hook(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                         const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                         const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                         const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* out, float* mass) {
    {
        // round-3 path: stand-alone producer (qkv_pack + cross_pack, L = 1) then the DMA + MFMA kernel, at the SITE_ATTN precision
        const int D = H * dh, dhp = dh <= 64 ? 64 : 128, Np = pad8(N), Rp = pad8(R > 0 ? R : 0), Cp = Rp + pad8(P > 0 ? P : 0);
        const int pa = E.site_precision(Engine::SITE_ATTN);
        const size_t nqk = (size_t)B * H * N * dhp, nvt = (size_t)B * H * dhp * Np, ng = (size_t)B * N * D, nc = (size_t)B * H * Cp * dhp;
        const int nr = N * rot_dim;
        bf16_t* img = nullptr; float *rc = nullptr, *rs = nullptr; bf16_t* ob = nullptr;
        const size_t tot = 2 * (2 * nqk + nvt + ng + 2 * nc) + 64;
        if (hipMalloc(&img, tot * 2) != hipSuccess || hipMalloc(&rc, (size_t)(nr + 4) * 4) != hipSuccess ||
            hipMalloc(&rs, (size_t)(nr + 4) * 4) != hipSuccess || hipMalloc(&ob, (size_t)B * N * D * 2 * 2 + 64) != hipSuccess)
            return E.fail("test_attention_mfma: alloc failed");
        (void)hipMemsetAsync(img, 0, tot * 2, ST(stream));
        (void)launch_rope_cossin(rope, rc, rs, nr, ST(stream));
        bf16_t* p = img;
        auto take = [&](size_t n) { bf16_t* r = p; p += (n + 7) & ~size_t(7); return r; };
        QkvPackArgs pk{};
        pk.qkvg = qkvg; pk.qw = qw; pk.kw = kw; pk.eps = eps; pk.q_scale = 1.0f / sqrtf((float)dh);
        pk.rope_cos = rc; pk.rope_sin = rs; pk.rot_dim = rot_dim; pk.prec = pa;
        pk.q = take(nqk); pk.q_lo = take(nqk); pk.k = take(nqk); pk.k_lo = take(nqk); pk.vt = take(nvt); pk.vt_lo = take(nvt);
        pk.g = take(ng); pk.g_lo = take(ng);
        pk.B = B; pk.N = N; pk.H = H; pk.dh = dh; pk.dhp = dhp; pk.Np = Np;
        hipError_t e = launch_qkv_pack(pk, ST(stream));
        AttnImg ai{};
        ai.prec = pa;
        ai.q = pk.q; ai.q_lo = pk.q_lo; ai.k = pk.k; ai.k_lo = pk.k_lo; ai.vt = pk.vt; ai.vt_lo = pk.vt_lo; ai.g = pk.g; ai.g_lo = sm_lo_for(pa, pk.g_lo);
        if (Cp > 0 && e == hipSuccess) {
            CrossPackArgs cp{};
            cp.k_ref = k_ref; cp.v_ref = v_ref; cp.k_text = k_text; cp.v_text = v_text;
            cp.kc = take(nc); cp.kc_lo = take(nc); cp.vtc = take(nc); cp.vtc_lo = take(nc);
            cp.prec = pa; cp.L = 1; cp.B = B; cp.H = H; cp.dh = dh; cp.dhp = dhp; cp.R = R > 0 ? R : 0; cp.P = P > 0 ? P : 0; cp.Rp = Rp; cp.Cp = Cp;
            e = launch_cross_pack(cp, ST(stream));
            ai.kc = cp.kc; ai.kc_lo = cp.kc_lo; ai.vtc = cp.vtc; ai.vtc_lo = cp.vtc_lo;
        }
        ai.mask_self = mask_self; ai.mask_ref = mask_ref; ai.mask_text = mask_text;
        ai.out_hi = ob; ai.out_lo = ob + (((size_t)B * N * D + 7) & ~size_t(7)); ai.ors = D;   // split pair: hi + lo ~ fp32
        ai.B = B; ai.N = N; ai.H = H; ai.dh = dh; ai.Np = Np; ai.R = R > 0 ? R : 0; ai.P = P > 0 ? P : 0; ai.Rp = Rp; ai.Cp = Cp;
        if (e == hipSuccess && out) e = launch_attention_img(ai, ST(stream));
        if (e == hipSuccess && out) e = launch_split_to_f32(ai.out_hi, ai.out_lo, out, (long)B * N * D, ST(stream));
        if (e == hipSuccess && mass) e = launch_attn_text_mass(ai, mass, B, H >= 32 ? ~0u : (1u << H) - 1u, 1.0f / (float)H, 1, ST(stream));
        (void)hipStreamSynchronize(ST(stream));
        (void)hipFree(img); (void)hipFree(rc); (void)hipFree(rs); (void)hipFree(ob);
        return e == hipSuccess ? 0 : E.fail_hip(e, mass ? "attn_text_mass" : "attention_img");
    }
}

extern "C" {

int smtts_test_attention_mfma(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                              const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                              const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                              const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* out) { NULLCHK;
    return attn_img_hook(h, stream, qkvg, qw, kw, eps, rope, rot_dim, k_ref, v_ref, R, k_text, v_text, P, mask_self, mask_ref, mask_text,
                         B, N, H, dh, out, nullptr);
}
int smtts_test_attn_text_mass(smtts_handle h, void* stream, const float* qkvg, const float* qw, const float* kw, float eps,
                              const float* rope, int rot_dim, const float* k_ref, const float* v_ref, int R,
                              const float* k_text, const float* v_text, int P, const uint8_t* mask_self,
                              const uint8_t* mask_ref, const uint8_t* mask_text, int B, int N, int H, int dh, float* mass) { NULLCHK;
    if (!mass || P <= 0 || !k_text || B <= 0 || N <= 0) return E.fail("test_attn_text_mass: needs text keys and an output (B, N, P > 0)");
    return attn_img_hook(h, stream, qkvg, qw, kw, eps, rope, rot_dim, k_ref, v_ref, R, k_text, v_text, P, mask_self, mask_ref, mask_text,
                         B, N, H, dh, nullptr, mass);
}

}  // extern "C"
