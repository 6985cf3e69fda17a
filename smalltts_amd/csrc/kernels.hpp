// Launchers for the non-GEMM kernels of the smalltts gfx950 library (definitions in kernels.hip,
// attention.hip, codec_kernels.hip).  All pointers are device pointers; all launches are async on `st`.
#pragma once
#include "common.hpp"

// y[m][c] = LN(x[m][:]; eps, no affine)[c] * (1 + scale[r][c]) + shift[r][c],  r = mod_row0 + (m / rows_per_batch) * mod_rstride
// (reference dit.py:19-25, 197-199, 35-39).  shift/scale are rows of the modulation table (ld = mod_ld).
// Output: fp32 `y`, or (when yhi != null) the split bf16 pair yhi/ylo that feeds gemm3 directly.
hipError_t launch_ln_modulate(const float* x, float* y, bf16_t* yhi, bf16_t* ylo, int M, int C, float eps,
                              const float* shift, const float* scale, long mod_ld, int mod_row0, int mod_rstride,
                              int rows_per_batch, hipStream_t st, float* mean_out = nullptr);   // mean_out [M]: the row means (may be null)

// y[m][c] = x[m][c] * rsqrt(mean(x[m][:]^2) + eps) * w[c]   (reference dit.py:42-53, 1-D weight).
// Rows are addressed through RowMaps so padded codec images can be normalised in place of a copy.
hipError_t launch_rmsnorm(const float* x, RowMap xmap, float* y, bf16_t* yhi, bf16_t* ylo, RowMap ymap, int M, int C,
                          float eps, const float* w, hipStream_t st);

// In-place per-head RMSNorm of the cross-K cache [L][B][H][S][dh] with weights [L][H][dh] (dit.py:83).
hipError_t launch_headnorm(float* k, int L, int B, int H, int S, int dh, float eps, const float* w, hipStream_t st);

struct AttnArgs {
    // self q/k/v/gate: element (b, n, h, d) at ptr[b*bs + n*rs + h*dh + d]
    const float* q;
    const float* k;
    const float* v;
    const float* gate;  // same addressing; out *= sigmoid(gate)
    long bs, rs;
    const float* qw;  // [H][dh] RMSNorm weights (q_norm / k_norm)
    const float* kw;
    float eps;
    const float* rope_cos;  // cos / sin of the angle table [pos][rot_dim] (a0 a0 a1 a1 ..., reference
    const float* rope_sin;  // infer/onnx.py:42-47), precomputed by launch_rope_cossin
    int rot_dim;        // rotated leading dims (64 for DiT, dh for the encoders)
    // cross keys (may be null / 0): [b][h][j][d] contiguous
    const float* k_ref; const float* v_ref; int R;
    const float* k_text; const float* v_text; int P;
    const uint8_t* mask_self;  // [B][N]  key validity (may be null = all valid)
    const uint8_t* mask_ref;   // [B][R]
    const uint8_t* mask_text;  // [B][P]
    int prenormed;      // 1: q and k were already RMS-normalised + rotated in place by launch_qk_prep (0: the kernel does it on the fly)
    float* out; long obs, ors;  // out (b, n, h*dh + d)
    bf16_t* out_hi; bf16_t* out_lo;  // when out_hi != null the result is written as a split bf16 pair instead
    int B, N, H, dh;
};
// fp32 VALU attention (attention.hip): the A/B reference of the DMA + MFMA kernel below (test hook, SMTTS_ATTN_IMG=0)
hipError_t launch_attention(const AttnArgs& a, hipStream_t st);
// In place on the packed projection buffer: q <- RoPE(RMSNorm_head(q) * qw), k <- RoPE(RMSNorm_head(k) * kw)
// (dit.py:95-108); one wave per (row, head, q|k).  Uses the q/k/bs/rs/qw/kw/eps/rope/rot_dim/B/N/H/dh fields.
hipError_t launch_qk_prep(const AttnArgs& a, hipStream_t st);

// ---- attention on producer-written operand images (attention_img.hip) -----------------------------------------------------------
// Every array is a 16-bit GEMM-operand array in format `prec` (PREC_F16 / PREC_BF16: `*_lo` unused; PREC_BF16X3: hi + lo pair).
static inline int pad8(int n) { return (n + 7) & ~7; }
struct AttnImg {
    int prec;
    const bf16_t *q, *q_lo;      // [B][H][N][DHP]   RMSNorm_head * w, RoPE, x 1/sqrt(dh)   (DHP = 64 / 128, pad dims zero)
    const bf16_t *k, *k_lo;      // [B][H][N][DHP]   self keys, normalised + rotated
    const bf16_t *vt, *vt_lo;    // [B][H][DHP][Np]  self values transposed, Np = pad8(N), columns >= N zero
    const bf16_t *g, *g_lo;      // [B*N][H*dh]      sigmoid(gate)
    const bf16_t *kc, *kc_lo;    // [B][H][Cp][DHP]  cross keys of this layer (null: self-attention only), pad rows zero
    const bf16_t *vtc, *vtc_lo;  // [B][H][DHP][Cp]  cross values transposed; Cp = Rp + pad8(P), Rp = pad8(R)
    const uint8_t *mask_self, *mask_ref, *mask_text;   // [B][N], [B][R], [B][P] key validity (null = all valid)
    bf16_t *out_hi, *out_lo;     // o[(b*N + n)*ors + h*dh + d] in the format store_split4 derives from out_lo
    long ors;
    int B, N, H, dh, Np, R, P, Rp, Cp;
};
hipError_t launch_attention_img(const AttnImg& a, hipStream_t st);
// ---- word timings (align.hip) ---------------------------------------------------------------------------------------------------
// The text-attention tap: behind launch_attention_img(a), on the same images and masks.  mass f32 (rows, N, P) (+)= scale * sum over the
// heads in `heads` (bit h) of softmax(all valid keys)[text key p], for the first `rows` batch rows of a (the conditional rows of a CFG
// batch); first != 0 stores, else adds.  Exactly 0 for masked frames / text columns / rows without a valid key.  No atomics.
hipError_t launch_attn_text_mass(const AttnImg& a, float* mass, int rows, unsigned heads, float scale, int first, hipStream_t st);
// Monotone alignment of mass (B, N, P), one workgroup per row: frames [0, n_len[b]), tokens [p0[b], p1[b]) (DEVICE int32 arrays, clamped
// to the shape) -> spans int32 (B, P, 2) = (first, last) frame of every token on the path ((-1, -1) outside the range and for empty
// rows), score f32 (B) = the path cost (0 for empty rows).  N <= 225 and P <= 198 (back-pointers in LDS), else hipErrorInvalidValue.
hipError_t launch_align_path(const float* mass, int B, int N, int P, const int* n_len, const int* p0, const int* p1, int* spans, float* score,
                             hipStream_t st);
// ---- takes (takes.hip) ------------------------------------------------------------------------------------------------------------
// Quality score of every sampler row behind launch_align_path, one workgroup per row: feat int32 (B, 4) = (cells, skipped, longest, idle)
// and total f32 (B) = ((w0 c0 + w1 c1) + w2 c2) + w3 c3 from single rounded fp32 operations (the definitions: include/smalltts_hip.h
// smtts_take_scores); +inf and zero features for an empty row.  n_len / p0 / p1 as launch_align_path (DEVICE, clamped).  N <= 225, P <= 198.
hipError_t launch_take_scores(const float* mass, const int* spans, const float* path_score, const int* n_len, const int* p0, const int* p1,
                              int B, int N, int P, float tau_tok, float tau_frm, float w0, float w1, float w2, float w3, int* feat,
                              float* total, hipStream_t st);
// Rows piece-major (row = g * K + k, 1 <= K <= 16): the winner of group g is the lowest k with the smallest total (NaN counts as +inf);
// its rows of x (N, 64), n_len and, where given, spans (P, 2) and mass (N, P) are copied to row g of the outputs bit for bit, winner
// int32 (G) = k.  An optional input and its output are given or NULL together.
hipError_t launch_take_select(const float* total, int G, int K, int N, int P, const float* x, const int* n_len, const int* spans,
                              const float* mass, float* x_win, int* n_win, int* spans_win, float* mass_win, int* winner, hipStream_t st);
// ---- CTC (ctc.hip) ------------------------------------------------------------------------------------------------------------------
// nll f32 (B) = F.ctc_loss(blank 0, reduction 'none', zero_infinity False) of logp f32 (B, T, C) over the first t_len[b] frames against
// tokens[b][p0 : p1) (i32 (B, P); t_len into [0, T], p0 / p1 into [0, P], tokens into [1, C), all DEVICE, clamped); +inf for an empty or
// infeasible row.  One workgroup per row, thread = extended state.  T >= 1, 1 <= P <= 198, 2 <= C <= 256, else hipErrorInvalidValue.
hipError_t launch_ctc_score(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P, int C,
                            float* nll, hipStream_t st);
// per-frame argmax (lowest class on ties), runs collapsed, class 0 dropped -> ids i32 (B, T), zeros behind n_ids i32 (B).  1 <= T <= 4096.
hipError_t launch_ctc_greedy(const float* logp, const int* t_len, int B, int T, int C, int* ids, int* n_ids, hipStream_t st);
// the best path of ctc_score's lattice (same clamping): spans i32 (B, P, 2) = (first, last) frame of every token of the window, (-1, -1)
// outside it and on a row that is not aligned; tok_logp f32 (B, P) the path's log-probability per token; frame_tok i32 (B, T) or NULL the
// token of every label frame, -1 elsewhere; score f32 (B) the path's log-probability, -inf for an empty or infeasible row.  One workgroup
// per row, the 2-bit moves in dynamic LDS sized by T and P.  1 <= T <= 1024, 1 <= P <= 198, 2 <= C <= 256, else hipErrorInvalidValue.
hipError_t launch_ctc_align(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P, int C,
                            int* spans, float* tok_logp, int* frame_tok, float* score, hipStream_t st);
// ---- long CTC alignment (ctc_long.hip) -------------------------------------------------------------------------------------------------
// launch_ctc_align's definition and outputs for rows past its limits: delta in registers (32 states per thread), the 2-bit moves in the
// workspace table [t][thread], the trace through LDS in chunks of 256 steps.  ws: ctc_align_long_ws_bytes(B, T, P) bytes (a multiple of
// 256, 0 outside the range), 256-byte aligned, contents irrelevant.  1 <= T <= 65536, 1 <= P <= 16383, 2 <= C <= 256, else
// hipErrorInvalidValue.
size_t ctc_align_long_ws_bytes(int B, int T, int P);
hipError_t launch_ctc_align_long(const float* logp, const int* t_len, const int* tokens, const int* p0, const int* p1, int B, int T, int P,
                                 int C, int* spans, float* tok_logp, int* frame_tok, float* score, void* ws, hipStream_t st);
// ---- recogniser (asr.hip) -----------------------------------------------------------------------------------------------------------
// Device pointers of the packed recogniser weights (Engine::finalize_asr): every 64 x 64 block of a product's weight transposed to
// [k][n], 16-byte aligned; vectors as loaded.
struct AsrFfnW { const float *ln_w, *ln_b, *w1t /* [16][64 k][64 hidden] */, *b1, *w2t /* [16][64 hidden][64 n] */, *b2; };
struct AsrConvW {
    const float *ln_w, *ln_b, *pw1t /* [2][64][64]: value half, gate half */, *pw1b, *dw_w /* [64][9] */, *dw_b;
    const float *bn_scale, *bn_shift /* BatchNorm (eval) folded */, *pw2t, *pw2b;
};
struct AsrLayerW {
    AsrFfnW ffn1, ffn2;
    const float *aln_w, *aln_b, *wqkv_t /* [3][64][64] */, *bqkv, *wo_t, *bo;
    AsrConvW conv;
    const float *fln_w, *fln_b;
};
struct AsrW {
    const float *up_w /* [64][4] */, *up_b;
    AsrLayerW layer[7];
    const float *proj_t /* [4][64][64], classes >= 198 zero */, *proj_b /* [256] */;
};
size_t asr_ws_bytes(int B, int N);
// A tap sink (tests only; NULL in every product call, and then a launcher enqueues exactly its kernels).  When set, the launcher copies
// the whole per-call buffer each launch wrote into the sink's slot for that launch (hipMemcpyAsync on the same stream, right behind the
// launch, before a later launch overwrites the buffer): slot i is launch i, in launch order, at off[i] bytes behind base.
struct ScorerTaps { char* base; const size_t* off; };
constexpr int ASR_TAPS = 44, SV_TAPS = 23;
// bytes launch `slot` of a call writes into (the whole buffer, rows behind a row's length included); 0 outside [0, *_TAPS)
size_t asr_tap_bytes(int B, int N, int slot);
// x f32 (B, N, 64), n_len i32 (B) (clamped into [0, N]) -> logp f32 (B, 4 N, 198), 0.0 at and behind frame 4 n_b; ws: asr_ws_bytes, 256-byte
// aligned, may hold anything.  1 <= N <= 225.
hipError_t launch_asr_logprobs(const AsrW& w, const float* x, const int* n_len, int B, int N, void* ws, float* logp, hipStream_t st,
                               const ScorerTaps* taps = nullptr);
// ---- speaker verifier (sv.hip) ---------------------------------------------------------------------------------------------------------
// Device pointers of the packed verifier weights (Engine::finalize_sv).  A product's weight (n_out, k_in): 64 x 64 blocks, each transposed
// to [k][n], outputs outer, inputs inner; a k = 3 convolution has k_in = tap * channels + channel.  scale / shift: the BatchNorm (eval)
// behind the ReLU, folded; NULL where the product has none.
struct SvTdnnW { const float *wt, *b, *scale, *shift; };
struct SvBlockW {
    SvTdnnW tdnn1, band[11] /* each [3 taps * 64][64] */, tdnn2;
    const float *se_w1t /* [768][192] */, *se_b1, *se_w2t /* [192][768] */, *se_b2;
    int dil;
};
struct SvW {
    SvTdnnW in;      // blocks.0: 3 taps x 64 -> 768
    SvBlockW block[3];
    SvTdnnW mfa;     // 2304 -> 2304
    SvTdnnW att;     // the pooling's TDNN, columns [0, 2304) of its 6912: 2304 -> 192
    const float* att_ct /* its columns [2304, 6912) transposed: [4608][192] */;
    SvTdnnW logit;   // 192 -> 2304, bias only
    const float *pool_scale, *pool_shift /* asp_bn folded, 4608 */, *fc_t /* [4608][192] */, *fc_b;
};
size_t sv_ws_bytes(int B, int N);
// x f32 (B, N, 64), n_len i32 (B) (clamped into [0, N]) -> emb f32 (B, 192), every row as if alone in its batch; 0.0 for a row under 6
// frames.  ws: sv_ws_bytes, 256-byte aligned, may hold anything.  6 <= N <= 225, else hipErrorInvalidValue.
size_t sv_tap_bytes(int B, int N, int slot);   // as asr_tap_bytes
hipError_t launch_sv_embed(const SvW& w, const float* x, const int* n_len, int B, int N, void* ws, float* emb, hipStream_t st,
                           const ScorerTaps* taps = nullptr);
// cos f32 (B): row b of emb (B, D) against row b / K of ref (B / K, D), each norm clamped at 1e-8 (a zero row gives 0).  One wave per row.
hipError_t launch_sv_cosine(const float* emb, const float* ref, int B, int K, int D, float* cos, hipStream_t st);
// ---- repair (repair.hip) ----------------------------------------------------------------------------------------------------------
// Pin mask of every row behind launch_align_path, one workgroup per row: a token of [p0, p1) is bad when its span is empty, longer than
// max_span, or holds no frame with mass >= tau_tok; a bad token with a span frees its frames +- margin.  pin u8 (B, N) = 1 for frames
// below n that are not freed or that keep (u8 (B, N) or NULL) names, 0 elsewhere (every byte written); counts int32 (B, 2) = (bad
// tokens, frames below n with pin 0).  The definitions: include/smalltts_hip.h smtts_repair_plan.  N <= 225, P <= 198.
hipError_t launch_repair_plan(const float* mass, const int* spans, const int* n_len, const int* p0, const int* p1, const uint8_t* keep,
                              int B, int N, int P, float tau_tok, int max_span, int margin, uint8_t* pin, int* counts, hipStream_t st);
// Row g of x_new (N, 64) and, where given, spans_new (P, 2) and mass_new (N, P) replaces row g of the _cur buffers in place, bit for
// bit, where counts[g][1] > 0 and total_new[g] < total_cur[g] (NaN counts as +inf, strict <); total_out / feat_out (G) / (G, 4) are
// those of the row that stays, kept int32 (G) the decision.  The three small outputs must not alias an input.
hipError_t launch_repair_keep(int G, int N, int P, const float* total_cur, const float* total_new, const int* counts, const int* feat_cur,
                              const int* feat_new, float* x_cur, const float* x_new, int* spans_cur, const int* spans_new, float* mass_cur,
                              const float* mass_new, float* total_out, int* feat_out, int* kept, hipStream_t st);
// fp32 projection rows [B*N][4*H*dh] = [q | k | v | gate] (bias included) -> the self part of AttnImg (dit.py:95-108; the arithmetic
// the gemm3 EpiQKV epilogue performs on its accumulators, as a stand-alone kernel: test hook + reference for the epilogue)
struct QkvPackArgs {
    const float* qkvg;
    const float *qw, *kw;        // [H][dh]
    float eps, q_scale;
    const float *rope_cos, *rope_sin;   // [pos][rot_dim]
    int rot_dim, prec;
    bf16_t *q, *q_lo, *k, *k_lo, *vt, *vt_lo, *g, *g_lo;
    int B, N, H, dh, dhp, Np;
};
hipError_t launch_qkv_pack(const QkvPackArgs& p, hipStream_t st);
// fp32 cross-KV caches [L][B][H][R|P][dh] (the C ABI's rank-5 tensors) -> Kc [L][B][H][Cp][dhp], Vc^T [L][B][H][dhp][Cp]
struct CrossPackArgs {
    const float *k_ref, *v_ref, *k_text, *v_text;
    bf16_t *kc, *kc_lo, *vtc, *vtc_lo;
    int prec, L, B, H, dh, dhp, R, P, Rp, Cp;
};
hipError_t launch_cross_pack(const CrossPackArgs& p, hipStream_t st);
// out[i] = hi[i] + lo[i]  (an operand image back to fp32: test hooks; lo in the format encoding of common.hpp: split pair, fp16 tag or null = bf16)
hipError_t launch_split_to_f32(const bf16_t* hi, const bf16_t* lo, float* out, long n, hipStream_t st);

// out[m][:] = table[ids[m]][:]  (phonemes.py:201)
hipError_t launch_embedding(const int64_t* ids, const float* table, float* out, int M, int C, int vocab, hipStream_t st);

// e[r][i] = sin(1000 t[r] f_i) (i<128) | cos (i>=128), f_i = exp(-i ln(1e4)/127)   (model.py:23-28)
hipError_t launch_time_sinusoid(const float* t, float* e, int rows, hipStream_t st);

// mask[b][j] = j < min(len[b], R)   (style.py:155-162)
hipError_t launch_len_mask(const int64_t* len, uint8_t* mask, int B, int R, hipStream_t st);

// gm[(b*G+g)][pad + t][c] = mask[b][t] ? h[b][t][g*cpg + c] : 0 ; pad frames and c>=cpg are zero.
hipError_t launch_convpos_pack(const float* h, const uint8_t* mask, bf16_t* gm_hi, bf16_t* gm_lo, int B, int T, int G,
                               int cpg, int pad, int gstride, hipStream_t st);
// in place: table[r][c0 + c] = tanh(table[r][c0 + c]) for the two gate column blocks of every DiT block
// LN-fold tables (gemm.hpp LnFoldIn): for every sampler step (modulation-table row) and every AdaLN'd GEMM site of the DiT blocks,
//   tab[row][0][off + n] = sum_k W[n][k] shift[k],   tab[row][1][off + n] = sum_k W[n][k] (1 + scale[k])        (K = 960)
// with W the 16-bit weights the GEMM itself multiplies (fmt 0: one fp16 array, 1: bf16 hi (+ lo when non-null)).
struct FoldSite { const bf16_t* w; const bf16_t* wlo; int N; int fmt; int shift_off, scale_off; long out_off; };
struct FoldSites { FoldSite s[24]; int n; long NF; };
hipError_t launch_fold_vectors(const FoldSites& sites, const float* mod, long mod_ld, int rows, float* tab, hipStream_t st);
hipError_t launch_tanh_gates(float* mod, int rows, long ld, int n_blocks, int per_block, int hidden, hipStream_t st);
// fp32 -> split bf16 pair, rows addressed through RowMaps (element offsets)
hipError_t launch_to_split(const float* x, RowMap xmap, bf16_t* hi, bf16_t* lo, RowMap omap, int M, int C, hipStream_t st);

// sampler element-wise steps (infer/onnx.py:105,125 ; teacher ODE see DESIGN.md)
hipError_t launch_axpby(float* out, const float* x, const float* y, float a, float b, long n, hipStream_t st);
// pinned sampling: axpby with a per-frame select (frame = 64 floats, K = pin && mask; 16-byte aligned buffers).  renoise: x_t = a x + s eps
// with x from `x` (src 0), K ? x_pin : 0 (src 1) or x_pin (src 2); update: x = K ? x_pin : a x_t + b v.
hipError_t launch_pin_renoise(float* xt, const float* x, const float* x_pin, const uint8_t* pin, const uint8_t* mask, const float* eps,
                              float a, float s, int src, long n, hipStream_t st);
hipError_t launch_pin_update(float* x, const float* xt, const float* v, const float* x_pin, const uint8_t* pin, const uint8_t* mask,
                             float a, float b, long n, hipStream_t st);
// x0 = a*xt - s*v ; eps = s*xt + a*v ; xt_next = a2*x0 + s2*eps    (x0 written to x0_out)
hipError_t launch_ode_step(float* xt, const float* v, float* x0_out, float a, float s, float a2, float s2, long n,
                           hipStream_t st);
// v = vc + st*(vc - vt) + ss*(vc - vs) over [3][n] stacked velocities (distill.py:101-105)
hipError_t launch_cfg_combine(const float* v3, float* v, float s_text, float s_spk, long n, hipStream_t st);

// Philox4x32-10 + Box-Muller standard normals; element i uses counter (i/4, stream, 0, 0), key (seed lo, hi).
hipError_t launch_randn(float* out, long n, uint64_t seed, uint64_t stream, hipStream_t st);
// out (n_steps, B, Nmax, 64): row b of step s = launch_randn(n[b] * 64, seeds[b], s) then zeros; seeds / n: device arrays of B entries
hipError_t launch_randn_rows(float* out, const uint64_t* seeds, const int64_t* n, int n_steps, int B, int Nmax, hipStream_t st);

// synthetic weights (smalltts_amd/weights.py recipe, bit-exact)
hipError_t launch_synth(float* out, long n, uint64_t key, float mean, float half_range, hipStream_t st);
// fp32 -> GEMM weight arrays with optional row permutation/packing: dst row r <- src row perm[r] (perm null = identity).
// (hi, lo): bf16 split pair (or a single array, see common.hpp); h16 (optional): the same rows as fp16 for PREC_F16 sites
hipError_t launch_split_rows(const float* src, long src_ld, bf16_t* hi, bf16_t* lo, long dst_ld, int rows, int cols,
                             const int* perm, hipStream_t st, bf16_t* h16 = nullptr);
// l16 = fp16(src - float(h16)) over [rows][cols] (dst row stride dst_ld): low half of the fp16 weight pair of PREC_F16X2
hipError_t launch_f16_residual(const float* src, long src_ld, const bf16_t* h16, bf16_t* l16, long dst_ld, int rows, int cols, hipStream_t st);
// out2[0] = max_j (sqrt(C) ||W1_j o g|| + |b1_j|), out2[1] = sqrt(C) max |g|   (out2 zeroed by the caller; g / b1 may be null)
hipError_t launch_ffn_range_bound(const float* w1, const float* b1, const float* g, int F, int C, float* out2, hipStream_t st);
hipError_t launch_fill(float* p, float v, long n, hipStream_t st);
hipError_t launch_copy_strided(const float* src, long sld, float* dst, long dld, int rows, int cols, hipStream_t st);
// dst[n][k] (fp32, row-major N x K) = src[base + n1*sn1 + n0*sn0 + k1*sk1 + k0*sk0]  if k0 < k0valid else 0
// with n1 = n / n0dim, n0 = n % n0dim, k1 = k / k0dim, k0 = k % k0dim.  Covers the conv->GEMM weight re-layouts.
struct GatherSpec { long base, sn1, sn0, sk1, sk0; int n0dim, k0dim, k0valid; };
hipError_t launch_gather_pack(const float* src, float* dst, int N, int K, GatherSpec g, hipStream_t st);
// tab[pos][d] = pos * theta^(-(d & ~1)/dim)   pos < npos, d < dim   (rope angle tables; dit.py:138-149, style.py:13-18)
hipError_t launch_rope_table(float* tab, int npos, int dim, hipStream_t st);
// c[i] = cos(ang[i]), s[i] = sin(ang[i])
hipError_t launch_rope_cossin(const float* ang, float* c, float* s, int n, hipStream_t st);

// ---- codec element-wise kernels (channels-last padded images [B][pad + T][C]) -------------------
// x[b][t][c] += gamma[c] * (sum_k w[c][k] * n[b][t - (K-1) + k][c] + bias[c])   (causal depthwise conv)
hipError_t launch_dwconv_resid(float* x, const float* n, const float* w, const float* bias, const float* gamma,
                               int B, int T, int C, int K, int pad, hipStream_t st);
// dwconv_resid + the RMSNorm (weight norm_w) of the updated rows written as a split bf16 pair (the next GEMM's A operand)
// wide-stage codec mixer + the FFN's RMSNorm in one pass (kernels.hip mixer_wide_kernel): xin -> xout (another image), n2 = 16-bit rows [B*T][C]
bool mixer_wide_ok(int C, int K);
hipError_t launch_mixer_wide(const float* xin, float* xout, const float* norm_w, const float* w, const float* bias, const float* gamma,
                             const float* ffn_norm_w, bf16_t* n2hi, bf16_t* n2lo, int B, int T, int C, int K, int pad, float eps,
                             hipStream_t st);
hipError_t launch_dwconv_resid_rms(float* x, const float* n, const float* w, const float* bias, const float* gamma, int B, int T,
                                   int C, int K, int pad, float eps, const float* norm_w, bf16_t* yhi, bf16_t* ylo, RowMap ymap,
                                   hipStream_t st);
// audio[b][t] = bias + sum_{k,c} w[k][c] * x[b][t - (K-1) + k][c]    (head conv, Cout = 1)
hipError_t launch_head_conv(const float* x, const float* w, float bias, float* audio, int B, int T, int C, int K,
                            int pad, hipStream_t st);
// x[b][pad+t][c] = bias[c] + sum_k w[c][k] * audio[b][t-(K-1)+k]   (encoder stem conv, Cin = 1)
hipError_t launch_stem_conv1(const float* audio, const float* w, const float* bias, float* x, int B, int T, int C,
                             int K, int pad, hipStream_t st);
hipError_t launch_zero_pad_frames(float* x, int B, int T, int C, int pad, hipStream_t st);
hipError_t launch_zero_pad_frames3(float* x0, float* x1, float* x2 /* may be null */, int B, int T, int C, int pad, hipStream_t st);
// streamed decode (codec_stream.hip): the 8 pad frames of img [B][8 + T][C] <- the boundary's [8][C] block (at byte `offset`) of slot
// slots[b] of the state pool, the block <- the last 8 frames the image now has behind it (T < 8: the old block moved up by T, then the
// chunk).  slots: DEVICE int64 (B), each slot at most once, clamped into [0, n_slots).  img, pool, slot_stride, offset: 16-byte aligned
hipError_t launch_carry_frames(float* img, int B, int T, int C, void* pool, long slot_stride, long offset, long n_slots,
                               const int64_t* slots, hipStream_t st);

// Fused codec FFN block for C in {32, 64, 128}: x += gamma * (W2 gelu(W1 rmsnorm(x) + b1) + b2), hidden kept in LDS.
// w1 packed [F][CP], w2 packed [CP][F] with CP = max(C, 64) (zero padded).  (codec_ffn.hip)
// C in {32, 64}: weights LDS-resident, wave-autonomous (codec_ffn_wave.hip); w1 [F][ld1], w2 [>= C][F]
hipError_t launch_codec_ffn_wave(float* x, RowMap img, const float* norm_w, const bf16_t* w1hi, const bf16_t* w1lo, int ld1,
                                 const float* b1, const bf16_t* w2hi, const bf16_t* w2lo, const float* b2, const float* gamma,
                                 int M, int C, int F, float eps, int split, hipStream_t st, const LaunchTuning& tu);
// C in {32, 64}: mixer + FFN of one codec block in ONE pass over the image (codec_ffn_wave.hip, MIX kernels): xout = block(xin)
// all blocks of a C = 32 codec stage in one launch (codec_ffn_wave.hip, stage chain): per block the one-pass block's operands
struct CodecChainBlock {
    const float *mnorm_w, *dw_w, *dw_b, *mgamma, *norm_w;
    const bf16_t* w1; int ld1; const float* b1;
    const bf16_t* w2; const float *b2, *gamma;
};
bool codec_chain_wave_ok(int C, int F, int K, int T, int split, int nb);
hipError_t launch_codec_chain_wave(const float* xin, float* xout, RowMap img, const CodecChainBlock* blocks, int nb, int M, int C, int F, int K,
                                   float eps, int split, hipStream_t st, const LaunchTuning& tu);
bool codec_block_wave_ok(int C, int F, int K, int T, int split);
hipError_t launch_codec_block_wave(const float* xin, float* xout, RowMap img, const float* mnorm_w, const float* dw_w, const float* dw_b,
                                   const float* mgamma, const float* norm_w, const bf16_t* w1hi, const bf16_t* w1lo, int ld1,
                                   const float* b1, const bf16_t* w2hi, const bf16_t* w2lo, const float* b2, const float* gamma, int M,
                                   int C, int F, int K, float eps, int split, hipStream_t st, const LaunchTuning& tu);
// C in {128, 256}: weights streamed through an LDS ring (codec_ffn_stream.hip); w1 [F][C], w2t = launch_w2_tile_pack(W2 [C][F])
hipError_t launch_codec_ffn_stream(float* x, RowMap img, const float* norm_w, const bf16_t* w1hi, const bf16_t* w1lo,
                                   const float* b1, const bf16_t* w2thi, const bf16_t* w2tlo, const float* b2, const float* gamma,
                                   int M, int C, int F, float eps, int split, hipStream_t st, const LaunchTuning& tu);
hipError_t launch_w2_tile_pack(const bf16_t* in, bf16_t* out, int C, int F, hipStream_t st);



// x[m][n] += mask(m) * gate[(grow0 + (m / rows_per_batch) * grstride) * gld + n] * (sum_s part[s][m][n] + bias[n])
// (gate == null -> 1; fixed summation order s = 0..S-1).  Closes a split-K GEMM (see gemm3_resid_splitk).
// split-K reduce + gated residual, then LayerNorm * (1 + scale) + shift of the updated row -> split bf16 (the next AdaLN)
// Streaming ConvTranspose1d-as-GEMM for the two finest codec stages (W resident in LDS, one wave per 32 rows): codec_upsample.hip
bool codec_upsample_wave_ok(int K, int N);
hipError_t launch_codec_upsample_wave(const float* x, RowMap amap, const bf16_t* whi, const bf16_t* wlo, int ldw, const float* bias,
                                      float* out, RowMap omap, int M, int K, int N, int split, hipStream_t st, const LaunchTuning& tu);
hipError_t launch_splitk_resid_ln(const float* part, int S, float* x, const float* bias, const float* gate, long gld,
                                  int grow0, int grstride, int rows_per_batch, const uint8_t* rowmask, int M, int N, float eps,
                                  const float* shift, const float* scale, bf16_t* yhi, bf16_t* ylo, hipStream_t st,
                                  bool rms = false /* true: y = RMSNorm(x; weight = shift, eps), encoders */);
hipError_t launch_splitk_resid(const float* part, int S, float* x, const float* bias, const float* gate, long gld,
                               int grow0, int grstride, int rows_per_batch, const uint8_t* rowmask, int M, int N,
                               hipStream_t st, const RowMap* xmap = nullptr /* rows of x; default plain [M][N] */,
                               bool overwrite = false /* x = gate * (sum + bias) instead of x += ... */);

// Fused mixer for C <= 256 (out of place: tiles read K-1 halo frames that belong to the neighbouring tile, so the
// update cannot be done in place):  xout[b][t][c] = xin + gamma[c] * (bias[c] + sum_k w[k][c] * n[t-(K-1)+k][c]) with
// n = RMSNorm(xin; g, eps) recomputed in LDS for the tile + halo (x read once, written once).  Both images must have
// zero pad frames.
hipError_t launch_mixer_fused(const float* xin, float* xout, const float* norm_w, const float* w, const float* bias,
                              const float* gamma, int B, int T, int C, int K, int pad, float eps, hipStream_t st);

// device-side audio helpers (kernels.hip): polyphase resampler with a caller-built bank [up][klen], float -> PCM16
hipError_t launch_resample_poly(const float* x, long n_in, const float* bank, int up, int down, int klen, int width, float* y,
                                long n_out, int channels, hipStream_t st);
hipError_t launch_pcm16(const float* x, int16_t* y, long n, hipStream_t st);
// long-form synthesis (kernels.hip).  voice_expand: table [B][3] int64 (k_ptr, v_ptr, R_b) of per-voice (12, 1, 8, R_b, 120) slabs ->
// k, v (12, B, 8, Rmax, 120) with zeros past R_b, mask (B, Rmax).  stitch: rows x[b][0 .. len[b]) of a decoded batch, faded at both
// ends by the table w[F], to y[off[b] ..] (fp32, or PCM16 with launch_pcm16's arithmetic); max_len >= every len[b] sizes the grid and
// a row never reads past it; samples outside [0, y_n) are dropped
hipError_t launch_voice_expand(const int64_t* table, float* k, float* v, uint8_t* mask, int B, int Rmax, hipStream_t st);
hipError_t launch_stitch(const float* x, long x_stride, const int64_t* len, const int64_t* off, const float* w, int F, float* y, long y_n,
                         int B, long max_len, hipStream_t st);
hipError_t launch_stitch_pcm16(const float* x, long x_stride, const int64_t* len, const int64_t* off, const float* w, int F, int16_t* y,
                               long y_n, int B, long max_len, hipStream_t st);
// stitch with a source window and an optional gain per row: seg [B][2] int64 (start, n) clamped into the row, gain [B] or null
hipError_t launch_stitch_seg(const float* x, long x_stride, const int64_t* seg, const float* gain, const int64_t* off, const float* w, int F,
                             void* y, long y_n, int pcm16, int B, long max_len, hipStream_t st);
// endpoints of the speech in each row (two launches: frame_energy, endpoint_decide): e, pk [B][ceil(x_stride / W)] per-frame mean power
// and peak (written for frames of the row, untouched behind), seg [B][2] = (start, n), gain [B]; W % 4 == 0, 1 <= min_run <= 16
hipError_t launch_endpoints(const float* x, long x_stride, const int64_t* len, int W, float rel_pow, float floor_pow, int min_run, int lead,
                            int tail, float target_rms, float peak_limit, float max_gain, float* e, float* pk, int64_t* seg, float* gain,
                            int B, hipStream_t st);
// t[i] = float32(np.linspace(1, 0, n))[i] on the device (sampler timesteps)
hipError_t launch_linspace10(float* t, int n, hipStream_t st);
