// Engine, the DiT side: the condition encoders, the modulation and LN-fold tables, the denoiser and the samplers.
#include "engine_impl.hpp"

// ---------------------------------------------------------------------------------------------
// K10: encoder stack (style.py:70-105 / phonemes.py:131-167), x (fp32 residual) updated in place.
// GEMM inputs (y, o, ffh) live as split bf16 pairs written by the producing kernel.
// ---------------------------------------------------------------------------------------------
int Engine::enc_blocks(hipStream_t st, const EncoderW& e, const EncWs& w, int l0, int l1, int B, int S, const uint8_t* key_mask,
                       bool fold, int ks) {
    // On return w.y holds RMSNorm(x; norm of block l1, or final_norm) as a split pair: every norm except the first is fused into the
    // split-K reduction of the residual GEMM in front of it (the tiny-M projections get 4x the workgroups that way).
    const int M = B * S, D = e.dim;
    const RowMap rd = rowmap_plain(D);
    if (e.blocks.empty()) return fail("encoder without blocks");
    const int pe = prec_[SITE_ENCODER];
    unsigned* const se = satp(SITE_ENCODER);
    const SplitBuf y = w.y.as(pe, se), o = w.o.as(pe, se), ffh = w.ffh.as(pe, se);  // every activation here feeds a SITE_ENCODER GEMM
    HIPC(launch_rmsnorm(w.x, rd, nullptr, y.hi, y.lo, rd, M, D, e.eps, e.blocks[l0].an, st));
    // RMSNorm fold (gemm.hpp LnFoldIn, rms): the norm between two block GEMMs lives in their epilogues — the producer writes x w and the
    // row's sum-of-squares partials, the consumer scales by rstd; the first norm (above) and the final one (feeds a plain projection) stay
    // (fold needs D % 64 == 0: the consumer reads the D / 32 partials in pairs)
    LnFoldIn fin;
    fin.part = w.lnpart; fin.NP = D / 32; fin.inv_c = 1.0f / D; fin.eps = e.eps; fin.rms = 1;
    const size_t L = e.blocks.size();
    for (size_t l = l0; l < (size_t)l1; ++l) {
        const EncBlockW& b = e.blocks[l];
        const bool epi = attn_img_ && attn_epi_;   // the GEMM's own epilogue writes the attention operands
        if (!epi) HIPC(gemm3_store(ops3(w.y, rd, b.qkvg, M, pe), ACT_NONE, store_to(w.qkvg, rowmap_plain(4 * D), nullptr), 1, pe, st, tune_));
        AttnArgs a{};
        a.q = w.qkvg; a.k = w.qkvg + D; a.v = w.qkvg + 2 * D; a.gate = w.qkvg + 3 * D;
        a.bs = (long)S * 4 * D; a.rs = 4 * D;
        a.qw = b.qn; a.kw = b.kn; a.eps = e.eps;
        a.rope_cos = e.rope_cos; a.rope_sin = e.rope_sin; a.rot_dim = e.dh;
        a.mask_self = key_mask;
        a.out = nullptr; a.out_hi = o.hi; a.out_lo = o.lo; a.obs = (long)S * D; a.ors = D;
        a.B = B; a.N = S; a.H = e.heads; a.dh = e.dh;
        if (attn_img_) {
            // q / k head-norm + RoPE + operand formatting by the producer, then a DMA + MFMA attention kernel (attention_img.hip)
            const int pa = prec_[SITE_ATTN], Sp = pad8(S);
            QkvPackArgs pk{};
            pk.qkvg = w.qkvg; pk.qw = b.qn; pk.kw = b.kn; pk.eps = e.eps; pk.q_scale = 1.0f / sqrtf((float)e.dh);
            pk.rope_cos = e.rope_cos; pk.rope_sin = e.rope_sin; pk.rot_dim = e.dh; pk.prec = pa;
            pk.q = w.qi.hi; pk.q_lo = img_lo(pa, w.qi.lo); pk.k = w.ki.hi; pk.k_lo = img_lo(pa, w.ki.lo); pk.vt = w.vti.hi; pk.vt_lo = img_lo(pa, w.vti.lo);
            pk.g = w.gi.hi; pk.g_lo = img_lo(pa, w.gi.lo);
            pk.B = B; pk.N = S; pk.H = e.heads; pk.dh = e.dh; pk.dhp = e.dh <= 64 ? 64 : 128; pk.Np = Sp;
            if (l == (size_t)l0 && Sp != S) {   // pad key columns of V^T: zero once per call (the producer only writes n < S)
                HIPC(hipMemsetAsync(w.vti.hi, 0, (size_t)B * e.heads * pk.dhp * Sp * 2, st));
                if (pa == PREC_BF16X3) HIPC(hipMemsetAsync(w.vti.lo, 0, (size_t)B * e.heads * pk.dhp * Sp * 2, st));
            }
            if (epi) {
                EpiQKV eq{nullptr, pk.qw, pk.kw, pk.rope_cos, pk.rope_sin, pk.eps, pk.q_scale, pk.rot_dim, pa,
                          pk.q, pk.q_lo, pk.k, pk.k_lo, pk.vt, pk.vt_lo, pk.g, pk.g_lo, S, e.heads, e.dh, pk.dhp, Sp};
                if (fold && l > (size_t)l0) eq.fold = fin;   // w.y = x attention_norm.weight, written by the previous block's FF2 epilogue
                HIPC(gemm3_qkv(ops3(w.y, rd, b.qkvg, M, pe), eq, pe, st, tune_));   // (both encoders' heads are 64 / 128 wide: no padding)
            } else {
                HIPC(launch_qkv_pack(pk, st));
            }
            AttnImg ai{};
            ai.prec = pa;
            ai.q = pk.q; ai.q_lo = w.qi.lo; ai.k = pk.k; ai.k_lo = w.ki.lo; ai.vt = pk.vt; ai.vt_lo = w.vti.lo;   // (the consumer reads the lo ARRAYS, split format only)
            ai.g = pk.g; ai.g_lo = sm_lo_for(pa, w.gi.lo);
            ai.mask_self = key_mask;
            ai.out_hi = o.hi; ai.out_lo = o.lo; ai.ors = D;
            ai.B = B; ai.N = S; ai.H = e.heads; ai.dh = e.dh; ai.Np = Sp;
            HIPC(launch_attention_img(ai, st));
        } else {
#ifdef SMTTS_TEST_KERNELS   // the fp32 VALU reference attention (attention.hip): test builds only
            a.prenormed = 1;
            HIPC(launch_qk_prep(a, st));
            HIPC(launch_attention(a, st));
#else
            return fail("the fp32 VALU reference attention is not part of this build (make TEST_KERNELS=1)");
#endif
        }
        EpiResid<0> r1{w.x, rd, nullptr, nullptr, 0, 0, 0, 1, nullptr};
        NextLN n1{b.mn, nullptr, y.hi, y.lo, true, e.eps};
        if (fold) {
            EpiResidLN e1{w.x, rd, nullptr, nullptr, nullptr, b.mn, y.hi, y.lo, D, w.lnpart, D / 32, 1};
            HIPC(gemm3_resid_ln(ops3(w.o, rd, b.wo, M, pe), e1, pe, st, tune_));
        } else if (ks > 1) {
            HIPC(gemm3_resid_splitk(ops3(w.o, rd, b.wo, M, pe), r1, w.part, ks, pe, st, tune_, n1));
        } else {
            HIPC(gemm3_resid(ops3(w.o, rd, b.wo, M, pe), 0, r1, pe, st, tune_));
            HIPC(launch_rmsnorm(w.x, rd, nullptr, y.hi, y.lo, rd, M, D, e.eps, n1.shift, st));
        }
        EpiSwiGLU sw{nullptr, e.ff, nullptr, nullptr, ffh.hi, ffh.lo};
        if (fold) sw.fold = fin;
        HIPC(gemm3_swiglu(ops3(w.y, rd, b.ff13, M, pe), sw, pe, st, tune_));
        NextLN n2{l + 1 < L ? e.blocks[l + 1].an : e.final_norm, nullptr, y.hi, y.lo, true, e.eps};
        if (fold && l + 1 < L) {
            EpiResidLN e2{w.x, rd, nullptr, nullptr, nullptr, e.blocks[l + 1].an, y.hi, y.lo, D, w.lnpart, D / 32, 1};
            HIPC(gemm3_resid_ln(ops3(w.ffh, rowmap_plain(e.ff), b.w2, M, pe), e2, pe, st, tune_));
        } else if (ks > 1) {
            HIPC(gemm3_resid_splitk(ops3(w.ffh, rowmap_plain(e.ff), b.w2, M, pe), r1, w.part, ks, pe, st, tune_, n2));
        } else {
            HIPC(gemm3_resid(ops3(w.ffh, rowmap_plain(e.ff), b.w2, M, pe), 0, r1, pe, st, tune_));
            HIPC(launch_rmsnorm(w.x, rd, nullptr, y.hi, y.lo, rd, M, D, e.eps, n2.shift, st));
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// E0: condition encoder (model.py:88-95)
// ---------------------------------------------------------------------------------------------
size_t Engine::cond_ws_bytes(int B, int R, int P) const {
    Bump b(nullptr);
    EncWs ws, wt;  // the style and the text encoder run concurrently: one workspace each
    ws.plan(b, B, R);
    wt.plan(b, B, P);
    return b.off + 256;
}

// Side stream for the text-encoder half of cond_encode: forked from / joined into the caller's stream with
// events, so the caller still sees a single-stream operator.  Both encoders are tiny-M launch chains (120 / 240
// rows) that each fill a fraction of the chip; run side by side they overlap almost completely.
// One side stream + event pair PER CALLER STREAM (round 6): a caller that keeps several batches in flight gives each its own stream, and
// each of those forks onto its own side stream — the text encoders / modulation chains of batches in flight no longer queue behind one
// another on a single engine-wide stream.  A set enters the map only complete (stream and both events), at most 64 of them.
const Engine::AuxSet* Engine::side_set(hipStream_t st) {
    const auto it = aux_sets_.find(st);
    if (it != aux_sets_.end()) return &it->second;
    if (aux_sets_.size() >= 64) { fail("side streams: more than 64 caller streams on one engine"); return nullptr; }
    AuxSet a;
    hipError_t e = hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a.fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a.join, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (a.fork) (void)hipEventDestroy(a.fork);
        if (a.stream) (void)hipStreamDestroy(a.stream);
        fail_hip(e, "side stream / events of a caller stream");
        return nullptr;
    }
    return &aux_sets_.emplace(st, a).first->second;
}

int Engine::cond_encode(hipStream_t st, const float* ref, const int64_t* ref_len, const int64_t* ids,
                        const uint8_t* ph_mask, int B, int R, int P, float* k_ref, float* v_ref, uint8_t* ref_mask,
                        float* k_text, float* v_text, void* ws, size_t ws_bytes, float* ref_seq_out, float* mem_out) {
    ProfTag ptag("enc");
    if (!dit_ready_) return fail("cond_encode: DiT weights not finalized");
    if (R > kMaxPos || P > kMaxPos) return fail("cond_encode: sequence longer than the rope table (4096)");
    if (ws_bytes < cond_ws_bytes(B, R, P)) return fail("cond_encode: workspace too small");
    if (ws_misaligned(ws)) return fail("cond_encode: workspace must be 256-byte aligned");
    HIPC(hipSetDevice(device_));
    Bump bump(ws);
    EncWs w, wt;
    w.plan(bump, B, R);
    wt.plan(bump, B, P);
    const bool fork = dual_stream_ && R > 0 && P > 0;
    const AuxSet* const side = fork ? side_set(st) : nullptr;
    if (fork && !side) return 1;
    const hipStream_t stt = fork ? side->stream : st;  // stream of the text half
    if (fork) {
        HIPC(hipEventRecord(side->fork, st));  // inputs produced on the caller's stream are visible to the side stream
        HIPC(hipStreamWaitEvent(stt, side->fork, 0));
    }

    // ---- E2 text encoder (phonemes.py:200-207) + phoneme_proj (dit.py:293-298) ---------------
    const bool fold = fold_epi_on();
    if (P > 0) {
        if (text_in(stt, wt, ids, B, P)) return 1;
        if (enc_blocks(stt, text_, wt, 0, (int)text_.blocks.size(), B, P, ph_mask, fold && text_.dim % 64 == 0, ksplit_enc_)) return 1;
        float* mem = mem_out ? mem_out : wt.seq;
        if (enc_out(stt, true, wt, B * P, ph_mask, mem)) return 1;
        if (enc_kv(stt, true, wt, mem, B, P, k_text, v_text)) return 1;
    }
    if (fork) HIPC(hipEventRecord(side->join, stt));
    // ---- E1 style encoder (style.py:144-174) -------------------------------------------------
    if (R > 0) {
        HIPC(launch_len_mask(ref_len, ref_mask, B, R, st));
        if (style_in(st, w, ref, B, R)) return 1;
        if (enc_blocks(st, style_, w, 0, (int)style_.blocks.size(), B, R, ref_mask, fold && style_.dim % 64 == 0, ksplit_enc_)) return 1;
        float* seq = ref_seq_out ? ref_seq_out : w.seq;
        if (enc_out(st, false, w, B * R, ref_mask, seq)) return 1;
        // ---- E3 cross KV for the reference tokens (dit.py:80-93) -------------------------------
        if (enc_kv(st, false, w, seq, B, R, k_ref, v_ref)) return 1;
    }
    if (fork) HIPC(hipStreamWaitEvent(st, side->join, 0));  // join: everything after cond_encode sees both halves
    return 0;
}

// the encoders' stages (cond_encode): input, output projection, cross K / V of all 12 DiT blocks
int Engine::style_in(hipStream_t st, const EncWs& w, const float* ref, int B, int R) {
    HIPC(gemm_store(ops(ref, rowmap_plain(kLatent), style_in_, B * R), ACT_NONE,
                    store_to(w.x, rowmap_plain(512), rawp("style_encoder.in_proj.bias"), style_scale_), 1, prec_[SITE_COND], st, tune_));
    return 0;
}
int Engine::text_in(hipStream_t st, const EncWs& w, const int64_t* ids, int B, int P) {
    HIPC(launch_embedding(ids, rawp("phoneme_embedding.text_embedding.weight"), w.x, B * P, 512, 198, st));
    return 0;
}
int Engine::enc_out(hipStream_t st, bool text, const EncWs& w, int M, const uint8_t* key_mask, float* seq) {
    const int pe = prec_[SITE_ENCODER];
    HIPC(gemm3_store(ops3(w.y, rowmap_plain(512), text ? phproj_ : style_out_, M, pe), ACT_NONE,
                     store_to(seq, rowmap_plain(kHidden), rawp(text ? "dit.phoneme_proj.bias" : "style_encoder.out_proj.bias"), 1.f,
                              key_mask), 1, pe, st, tune_));
    return 0;
}
int Engine::enc_kv(hipStream_t st, bool text, const EncWs& w, const float* seq, int B, int S, float* k, float* v) {
    const int pk = prec_[SITE_CROSS_KV], M = B * S;
    const RowMap rh = rowmap_plain(kHidden);
    HIPC(launch_to_split(seq, rh, w.seqs.hi, w.seqs.as(pk, satp(SITE_CROSS_KV)).lo, rh, M, kHidden, st));
    EpiKV kv{k, v, text ? kvtext_b_ : kvref_b_, B, kHeads, kDh, S};
    HIPC(gemm3_kv(ops3(w.seqs, rh, text ? kvtext_ : kvref_, M, pk), kv, pk, st, tune_));
    HIPC(launch_headnorm(k, kBlocks, B, kHeads, S, kDh, 1e-6f, knc_, st));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// D1/D3/D5/D8 modulation table: all AdaLN vectors for `rows` distinct timesteps in one pass
//   mod[r] = [ blk0: shift_msa scale_msa tanh(gate_msa) shift_mlp scale_mlp tanh(gate_mlp) | ... | final: scale shift ]
// (tiny-M GEMM chain on the fp32-A kernel; the tanh of the gates, dit.py:198,201, is applied once here
// instead of per output element in the residual epilogues)
// ---------------------------------------------------------------------------------------------
int Engine::modulation(hipStream_t st, const float* t_dev, int rows, const ModWs& m) {
    ProfTag ptag("mod");
    const int pc = prec_[SITE_COND];  // tiny-M chain on the fp32-A kernel: always split-bf16 unless the preset is plain bf16
    HIPC(launch_time_sinusoid(t_dev, m.sinb, rows, st));
    HIPC(gemm_store(ops(m.sinb, rowmap_plain(256), time0_, rows), ACT_SILU,
                    store_to(m.t1, rowmap_plain(kHidden), rawp("time_embedding.mlp.0.bias")), 1, pc, st, tune_));
    HIPC(gemm_store(ops(m.t1, rowmap_plain(kHidden), time2_, rows), ACT_NONE,
                    store_to(m.temb, rowmap_plain(kHidden), rawp("time_embedding.mlp.2.bias")), 1, pc, st, tune_));
    HIPC(gemm_store(ops(m.temb, rowmap_plain(kHidden), emb0_, rows), ACT_SILU,
                    store_to(m.e1, rowmap_plain(2 * kHidden), rawp("dit.emb_proj.0.bias")), 1, pc, st, tune_));
    // AdaLN consumes silu(emb) only (dit.py:20,36), so the SiLU is fused into this epilogue
    HIPC(gemm_store(ops(m.e1, rowmap_plain(2 * kHidden), emb2_, rows), ACT_SILU,
                    store_to(m.semb, rowmap_plain(kHidden), rawp("dit.emb_proj.2.bias")), 1, pc, st, tune_));
    HIPC(gemm_store(ops(m.semb, rowmap_plain(kHidden), modall_, rows), ACT_NONE,
                    store_to(m.mod, rowmap_plain(kModLd), modall_b_), 1, pc, st, tune_));
    HIPC(launch_tanh_gates(m.mod, rows, kModLd, kBlocks, kModPerBlock, kHidden, st));
    return m.ftab ? fold_tables(st, m.mod, rows, m.ftab) : 0;
}

// LN-fold tables of every (step, block, site): W shift and W (1 + scale) on the weights the block GEMMs multiply
int Engine::fold_tables(hipStream_t st, const float* mod, int rows, float* ftab) {
    {
        const int pb = prec_[SITE_DIT_BLOCK];
        FoldSites fs{};
        fs.n = 0;
        fs.NF = kFoldNF;
        for (int l = 0; l < kBlocks; ++l) {
            const DitBlockW& b = blocks_[l];
            for (int site = 0; site < 2; ++site) {
                const PW& w = site ? b.ff13 : b.qkvgp;
                if (w.K != kHidden || w.N != (site ? 2 * kFF : 4 * kHeads * 128)) return fail("LN-fold: unexpected weight pack shape");
                FoldSite& f = fs.s[fs.n++];
                f.w = pb == PREC_F16 ? w.h16 : w.hi;
                f.wlo = pb == PREC_BF16X3 ? w.lo : nullptr;
                f.fmt = pb == PREC_F16 ? 0 : 1;
                f.N = w.N;
                f.shift_off = l * kModPerBlock + (site ? 3 : 0) * kHidden;
                f.scale_off = l * kModPerBlock + (site ? 4 : 1) * kHidden;
                f.out_off = l * kFoldPerBlock + (site ? 4L * kHeads * 128 : 0);
            }
        }
        HIPC(launch_fold_vectors(fs, mod, kModLd, rows, ftab, st));
    }
    return 0;
}

bool Engine::dit_fold_on(long rows) const { return fold_epi_on() && rows <= kFoldMaxRows; }

size_t Engine::dit_ws_bytes(int B, int N, int R, int P, int mod_rows, bool fold, int n_steps, int cfg) const {
    DitWs w;
    return w.plan(nullptr, B, N, R, P, mod_rows, fold, n_steps, cfg);
}

// What dit_blocks reads besides the residual stream, for the operators and the test hook alike.  rope: a caller-supplied angle table
// (reference operator input, infer/onnx.py:42-47,122), its cos / sin go into the workspace.
int Engine::dit_run(hipStream_t st, const CoreWs& w, const uint8_t* mask, const ModRow& row, const Cond& cond, const float* rope, int B,
                    int N, bool fold, bool unsplit, DitRun& d) {
    if (rope) HIPC(launch_rope_cossin(rope, w.rope_c, w.rope_s, N * 64, st));
    d.mask = mask; d.row = row; d.cond = &cond;
    d.rc = rope ? w.rope_c : rope_dit_cos_;
    d.rs = rope ? w.rope_s : rope_dit_sin_;
    d.frow = fold ? row.ftab + (long)row.row0 * 2 * kFoldNF : nullptr;   // [0]: W shift, [1]: W (1 + scale)
    d.ks_out = unsplit ? 1 : ksplit_out_;
    d.ks_ff2 = unsplit ? 1 : ksplit_ff2_;
    d.B = B; d.N = N;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// D0: one denoiser evaluation given a ready modulation table (model.py:97-100, dit.py:316-327)
// ---------------------------------------------------------------------------------------------
int Engine::denoise_core(hipStream_t st, const float* x_t, const uint8_t* mask, const ModRow& row, const Cond& cond, const float* rope,
                         int B, int N, float* velocity, const CoreWs& w, Call& call) {
    ProfTag ptag("dit");
    const int M = B * N;
    if (dit_embed(st, w, x_t, mask, B, N, !call.ws_zeroed)) return 1;
    // LN-fold (gemm.hpp LnFoldIn): inside the fused sampler — one modulation row for the whole batch, tables from modulation() —
    // the AdaLN between two block GEMMs lives in their epilogues (ftab: the tables sample() planned by the same predicate)
    const bool fold = row.ftab && row.rstride == 0 && dit_fold_on(M);
    // split-K exists to fill the chip at M = 600 (150 tiles of 64x64 for N = 960); the 3B-row CFG batches of the teacher
    // sampler (M = 1800: 435 tiles) fill it without, and the fused epilogue is cheaper than partials + reduce (495 -> 454 ms)
    // ... and so do several batches in flight (throughput tuning): there the unsplit GEMM + a separate AdaLN costs 2.3x fewer
    // workgroup-microseconds than three K slices + reduce, and that is what counts when other streams want the CUs
    static const bool splitk_tp = lab_env("SMTTS_SPLITK_TP") && atoi(lab_env("SMTTS_SPLITK_TP")) != 0;   // (A/B only)
    const bool unsplit = M > 1024 || (tuning_ == TUNE_THROUGHPUT && !splitk_tp);
    DitRun d;
    if (dit_run(st, w, mask, row, cond, rope, B, N, fold, unsplit, d)) return 1;
    HIPC(call.join());   // the modulation table may be on its way on the side stream (sample)
    if (dit_blocks(st, w, d, 0, kBlocks, call)) return 1;
    // the regions no kernel of this call writes (pad frames of the conv image, pad columns of the FF hidden, pad key columns of V^T)
    // are zeroed now: the sampler's later steps find them as the first step left them
    call.ws_zeroed = true;
    return dit_head(st, w, M, velocity);
}

// D2 input embedding (dit.py:246-253): h = proj(x); x = mask*mish(conv2(mask*mish(conv1(mask*h)))) + h   -> w.x (and w.h)
int Engine::dit_embed(hipStream_t st, const CoreWs& w, const float* x_t, const uint8_t* mask, int B, int N, bool init_ws) {
    const int M = B * N;
    const RowMap rh = rowmap_plain(kHidden);
    const int pc = prec_[SITE_COND], pcp = prec_[SITE_CONVPOS];
    const SplitBuf gm1 = w.gm1.as(pcp, satp(SITE_CONVPOS)), gm2 = w.gm2.as(pcp, satp(SITE_CONVPOS));
    HIPC(gemm_store(ops(x_t, rowmap_plain(kLatent), inproj_, M), ACT_NONE,
                    store_to(w.h, rh, rawp("dit.input_embed.proj.bias")), 1, pc, st, tune_));
    HIPC(launch_convpos_pack(w.h, mask, gm1.hi, gm1.lo, B, N, kConvG, kConvCpg, kConvPad, kConvGs, st));
    if (init_ws) {   // pad frames of the second conv's image (its producer writes the data frames only)
        HIPC(hipMemsetAsync(w.gm2.hi, 0, w.gm_elems * 2, st));
        if (pcp == PREC_BF16X3) HIPC(hipMemsetAsync(w.gm2.lo, 0, w.gm_elems * 2, st));
    }
    {
        // grouped conv k=31 as B*G small GEMMs: z = b*G + g, rows = frames, K = 31 taps x 64 (padded) channels
        // one product per GROUP over the rows of the whole batch (z = g, row m = (b, frame)): B * N rows fill their 64-row tiles
        // (600 rows: 94 %) where one product per (utterance, group) left the second tile of N = 75 rows at 11 of 64 (SMTTS_CONVPOS_BY_GROUP=0)
        const long zs = (long)(N + 2 * kConvPad) * kConvGs;
        const RowMap am = convpos_by_group_ ? rowmap_batched(kConvGs, N, (long)kConvG * zs, 0) : rowmap_plain(kConvGs);
        const int rows = convpos_by_group_ ? B * N : N, nz = convpos_by_group_ ? kConvG : B * kConvG;
        Gemm3Operands g = ops3(w.gm1, am, conv1_, rows, pcp, 0, kConvCpg);
        g.a_z = zs;
        g.w_z = (long)kConvCpg * conv1_.K;
        g.w_zmod = kConvG;
        EpiConvPos<0> e1{nullptr, nullptr, rawp("dit.input_embed.conv_pos_embed.conv1.bias"), mask, kConvG, kConvCpg, N,
                         kConvPad, kConvGs, gm2.hi, gm2.lo, convpos_by_group_ ? 1 : 0};
        HIPC(gemm3_convpos(g, false, e1, nz, pcp, st, tune_));
        g = ops3(w.gm2, am, conv2_, rows, pcp, 0, kConvCpg);
        g.a_z = zs;
        g.w_z = (long)kConvCpg * conv2_.K;
        g.w_zmod = kConvG;
        EpiConvPos<0> e2{w.x, w.h, rawp("dit.input_embed.conv_pos_embed.conv2.bias"), mask, kConvG, kConvCpg, N,
                         kConvPad, kConvGs, nullptr, nullptr, convpos_by_group_ ? 1 : 0};
        HIPC(gemm3_convpos(g, true, e2, nz, pcp, st, tune_));
    }
    return 0;
}

// D5-D8: DiT blocks [l0, l1) on the residual stream w.x (dit.py:189-212, 95-135)
int Engine::dit_blocks(hipStream_t st, const CoreWs& w, const DitRun& d, int l0, int l1, Call& call) {
    const int B = d.B, N = d.N, M = B * N;
    const Cond& c = *d.cond;
    const CrossImg& ci = c.img;
    const bool init_ws = !call.ws_zeroed;
    AlignTap& tap = call.tap;
    const RowMap rh = rowmap_plain(kHidden);
    const int pb = prec_[SITE_DIT_BLOCK], pc = prec_[SITE_COND];
    unsigned* const sb = satp(SITE_DIT_BLOCK);
    const SplitBuf yb = w.y.as(pb, sb), ob = w.o.as(pb, sb), ffh = w.ffh.as(pb, sb);
    if (!(attn_img_ && attn_epi_) && ensure_qkvg_unpadded()) return 1;
    // zero the padded tail columns [2400, 2432) of the FF hidden once per workspace use
    if (init_ws) {
        HIPC(hipMemsetAsync(w.ffh.hi, 0, (size_t)M * kFFp * 2, st));
        if (pb == PREC_BF16X3) HIPC(hipMemsetAsync(w.ffh.lo, 0, (size_t)M * kFFp * 2, st));
    }
    // The AdaLN in front of each GEMM is fused into the kernel that produced the residual stream it normalises
    // (split-K reduction + gated residual + LayerNorm-modulate in one pass); only the first one of the range runs alone.
    // LN-fold: the first AdaLN (here) and the final one (velocity head, SITE_COND precision) keep their ln_modulate, the first one
    // also writes the row means the producers shift by
    const bool fold = d.frow != nullptr;
    float* const lnc = fold && LN_FOLD_SHIFT ? w.lnc : nullptr;
    HIPC(launch_ln_modulate(w.x, nullptr, yb.hi, yb.lo, M, kHidden, 1e-6f, d.row.mod + (long)l0 * kModPerBlock + 0 * kHidden,
                            d.row.mod + (long)l0 * kModPerBlock + 1 * kHidden, kModLd, d.row.row0, d.row.rstride, N, st, lnc));
    const float* const mrow = d.row.mod + (long)d.row.row0 * kModLd;    // this step's modulation row (fold path only)
    auto fold_in = [&](int l, int site) {
        LnFoldIn f;
        f.part = w.lnpart; f.NP = kLnGroups; f.inv_c = 1.0f / kHidden; f.eps = 1e-6f;
        const long off = (long)l * kFoldPerBlock + (site ? 4L * kHeads * 128 : 0);
        f.wsh = d.frow + off;
        f.wc = d.frow + kFoldNF + off;
        f.cshift = lnc;
        f.nh = kFF;
        return f;
    };
    for (int l = l0; l < l1; ++l) {
        const DitBlockW& b = blocks_[l];
        const float* m = d.row.mod + (long)l * kModPerBlock;
        // D5 AdaLN-Zero (dit.py:19-25) already in w.y; D6 joint attention (dit.py:95-135)
        const bool epi = attn_img_ && attn_epi_;   // the GEMM's own epilogue writes the attention operands
        if (!epi)
            HIPC(gemm3_store(ops3(w.y, rh, b.qkvg, M, pb), ACT_NONE, store_to(w.qkvg, rowmap_plain(4 * kHidden), b.b_qkvg), 1,
                             pb, st, tune_));
        AttnArgs a{};
        a.q = w.qkvg; a.k = w.qkvg + kHidden; a.v = w.qkvg + 2 * kHidden; a.gate = w.qkvg + 3 * kHidden;
        a.bs = (long)N * 4 * kHidden; a.rs = 4 * kHidden;
        a.qw = b.qn; a.kw = b.kn; a.eps = 1e-6f;
        a.rope_cos = d.rc; a.rope_sin = d.rs; a.rot_dim = 64;
        const long lr = (long)l * B * kHeads * c.R * kDh, lp = (long)l * B * kHeads * c.P * kDh;
        a.k_ref = c.R > 0 ? c.k_ref + lr : nullptr; a.v_ref = c.R > 0 ? c.v_ref + lr : nullptr; a.R = c.R;
        a.k_text = c.P > 0 ? c.k_text + lp : nullptr; a.v_text = c.P > 0 ? c.v_text + lp : nullptr; a.P = c.P;
        a.mask_self = d.mask; a.mask_ref = c.ref_mask; a.mask_text = c.ph_mask;
        a.out = nullptr; a.out_hi = ob.hi; a.out_lo = ob.lo; a.obs = (long)N * kHidden; a.ors = kHidden;
        a.B = B; a.N = N; a.H = kHeads; a.dh = kDh;
        if (attn_img_) {
            const int pa = prec_[SITE_ATTN], Np = pad8(N);
            QkvPackArgs pk{};
            pk.qkvg = w.qkvg; pk.qw = b.qn; pk.kw = b.kn; pk.eps = 1e-6f; pk.q_scale = 1.0f / sqrtf((float)kDh);
            pk.rope_cos = d.rc; pk.rope_sin = d.rs; pk.rot_dim = 64; pk.prec = pa;
            pk.q = w.qi.hi; pk.q_lo = img_lo(pa, w.qi.lo); pk.k = w.ki.hi; pk.k_lo = img_lo(pa, w.ki.lo); pk.vt = w.vti.hi; pk.vt_lo = img_lo(pa, w.vti.lo);
            pk.g = w.gi.hi; pk.g_lo = img_lo(pa, w.gi.lo);
            pk.B = B; pk.N = N; pk.H = kHeads; pk.dh = kDh; pk.dhp = 128; pk.Np = Np;
            if (l == l0 && Np != N && init_ws) {   // pad key columns of V^T (the producer only writes n < N)
                HIPC(hipMemsetAsync(w.vti.hi, 0, w.vt_elems * 2, st));
                if (pa == PREC_BF16X3) HIPC(hipMemsetAsync(w.vti.lo, 0, w.vt_elems * 2, st));
            }
            if (epi) {
                EpiQKV eq{b.b_qkvgp, pk.qw, pk.kw, pk.rope_cos, pk.rope_sin, pk.eps, pk.q_scale, pk.rot_dim, pa,
                          pk.q, pk.q_lo, pk.k, pk.k_lo, pk.vt, pk.vt_lo, pk.g, pk.g_lo, N, kHeads, kDh, 128, Np};
                if (fold && l > l0) eq.fold = fold_in(l, 0);   // w.y = x (1 + scale_msa), written by the previous block's FF2 epilogue
                HIPC(gemm3_qkv(ops3(w.y, rh, b.qkvgp, M, pb), eq, pb, st, tune_));
            } else {
                HIPC(launch_qkv_pack(pk, st));
            }
            AttnImg ai{};
            ai.prec = pa;
            ai.q = pk.q; ai.q_lo = w.qi.lo; ai.k = pk.k; ai.k_lo = w.ki.lo; ai.vt = pk.vt; ai.vt_lo = w.vti.lo;   // (the consumer reads the lo ARRAYS, split format only)
            ai.g = pk.g; ai.g_lo = sm_lo_for(pa, w.gi.lo);
            if (ci.Cp > 0) {
                const long lc = (long)l * B * kHeads * ci.Cp * 128;
                ai.kc = ci.kc + lc; ai.vtc = ci.vtc + lc;
                if (pa == PREC_BF16X3) { ai.kc_lo = ci.kc_lo + lc; ai.vtc_lo = ci.vtc_lo + lc; }
            }
            ai.mask_self = d.mask; ai.mask_ref = c.ref_mask; ai.mask_text = c.ph_mask;
            ai.out_hi = ob.hi; ai.out_lo = ob.lo; ai.ors = kHidden;
            ai.B = B; ai.N = N; ai.H = kHeads; ai.dh = kDh; ai.Np = Np; ai.R = c.R; ai.P = c.P; ai.Rp = ci.Rp; ai.Cp = ci.Cp;
            HIPC(launch_attention_img(ai, st));
            if (tap.mass && tap.step_on && ((tap.layers >> l) & 1u)) {   // word timings: the text probabilities of this (step, layer)
                HIPC(launch_attn_text_mass(ai, tap.mass, tap.rows, tap.heads, tap.scale, tap.first ? 1 : 0, st));
                tap.first = false;
            }
        } else {
            if (tap.mass) return fail("the text-attention tap reads the attention operand images: not available with the image path switched off");
#ifdef SMTTS_TEST_KERNELS   // the fp32 VALU reference attention (attention.hip): test builds only
            a.prenormed = 1;
            HIPC(launch_qk_prep(a, st));
            HIPC(launch_attention(a, st));
#else
            return fail("the fp32 VALU reference attention is not part of this build (make TEST_KERNELS=1)");
#endif
        }
        // to_out + mask + gated residual (dit.py:117-118,198), then the MLP AdaLN (dit.py:199)
        EpiResid<0> r1{w.x, rh, nullptr, m + 2 * kHidden, kModLd, d.row.row0, d.row.rstride, N, d.mask};
        NextLN ln1{m + 3 * kHidden, m + 4 * kHidden, yb.hi, yb.lo};
        const float* const mr = mrow + (long)l * kModPerBlock;
        if (fold) {
            EpiResidLN e1{w.x, rh, nullptr, mr + 2 * kHidden, d.mask, mr + 4 * kHidden, yb.hi, yb.lo, kHidden, w.lnpart, kLnGroups, 0, lnc};
            HIPC(gemm3_resid_ln(ops3(w.o, rh, b.out, M, pb), e1, pb, st, tune_));
        } else if (d.ks_out > 1) {
            HIPC(gemm3_resid_splitk(ops3(w.o, rh, b.out, M, pb), r1, w.part, d.ks_out, pb, st, tune_, ln1));
        } else {
            HIPC(gemm3_resid(ops3(w.o, rh, b.out, M, pb), 1, r1, pb, st, tune_));
            HIPC(launch_ln_modulate(w.x, nullptr, ln1.yhi, ln1.ylo, M, kHidden, 1e-6f, ln1.shift, ln1.scale, kModLd, d.row.row0,
                                    d.row.rstride, N, st));
        }
        // D7 feed-forward (dit.py:199-201)
        EpiSwiGLU sw{nullptr, kFFp, b.b1, b.b3, ffh.hi, ffh.lo};
        if (fold) sw.fold = fold_in(l, 1);
        HIPC(gemm3_swiglu(ops3(w.y, rh, b.ff13, M, pb), sw, pb, st, tune_));
        // w2 + gated residual, then the next block's attention AdaLN — or D8's final AdaLN (chunk order scale, shift:
        // dit.py:37) after the last block
        EpiResid<0> r2{w.x, rh, b.b2, m + 5 * kHidden, kModLd, d.row.row0, d.row.rstride, N, nullptr};
        const float* mn = m + kModPerBlock;  // next block's modulation (or the final norm's [scale | shift])
        const SplitBuf yv = w.y.as(pc, satp(SITE_COND));  // the final AdaLN feeds the velocity head (SITE_COND)
        NextLN ln2 = l + 1 < kBlocks ? NextLN{mn + 0 * kHidden, mn + 1 * kHidden, yb.hi, yb.lo}
                                     : NextLN{mn + kHidden, mn, yv.hi, yv.lo};
        if (fold && l + 1 < kBlocks) {
            EpiResidLN e2{w.x, rh, b.b2, mr + 5 * kHidden, nullptr, mr + kModPerBlock + kHidden, yb.hi, yb.lo, kHidden, w.lnpart, kLnGroups, 0, lnc};
            HIPC(gemm3_resid_ln(ops3(w.ffh, rowmap_plain(kFFp), b.ff2, M, pb), e2, pb, st, tune_));
        } else if (d.ks_ff2 > 1) {
            HIPC(gemm3_resid_splitk(ops3(w.ffh, rowmap_plain(kFFp), b.ff2, M, pb), r2, w.part, d.ks_ff2, pb, st, tune_, ln2));
        } else {
            HIPC(gemm3_resid(ops3(w.ffh, rowmap_plain(kFFp), b.ff2, M, pb), 1, r2, pb, st, tune_));
            HIPC(launch_ln_modulate(w.x, nullptr, ln2.yhi, ln2.ylo, M, kHidden, 1e-6f, ln2.shift, ln2.scale, kModLd, d.row.row0,
                                    d.row.rstride, N, st));
        }
    }
    return 0;
}

// velocity head (model.py:100) on the final AdaLN image in w.y (SITE_COND format)
int Engine::dit_head(hipStream_t st, const CoreWs& w, int M, float* velocity) {
    const int pc = prec_[SITE_COND];
    HIPC(gemm3_store(ops3(w.y, rowmap_plain(kHidden), velocity_, M, pc), ACT_NONE,
                     store_to(velocity, rowmap_plain(kLatent), rawp("velocity.bias")), 1, pc, st, tune_));
    return 0;
}

// The unpadded QKVG pack of the DiT blocks, read by the A/B attention paths only: packed when one of them first runs (a test hook
// can flip the path after finalize), from the fp32 tensors that stay resident.  Synchronises the device: never on the product path.
int Engine::ensure_qkvg_unpadded() {
    if (blocks_.empty() || qkvg_unpadded_ready_) return 0;
    HIPC(hipDeviceSynchronize());
    struct PackMode { bool& f; bool old; explicit PackMode(bool& b) : f(b), old(b) { f = true; } ~PackMode() { f = old; } } pm(packing_);
    for (DitBlockW& b : blocks_) {
        if (b.qkvg.N) continue;   // (packed by finalize_dit when an A/B path was selected before it)
        b.qkvg = pack_rows({b.name + ".attn.to_q.weight", b.name + ".attn.to_k_self.weight", b.name + ".attn.to_v_self.weight",
                            b.name + ".attn.gate.weight"});
        if (!b.qkvg.N) {
            // a block failed (out of memory): nothing half-built may look finished to the next call — the packs made so far stay in
            // pack_allocs_ (freed by the next finalize) but are unlinked, and the flag stays down
            for (DitBlockW& c : blocks_) c.qkvg = PW();
            return fail("DiT block " + b.name + ": unpadded QKVG pack failed (" + err_ + ")");
        }
    }
    HIPC(hipDeviceSynchronize());
    qkvg_unpadded_ready_ = true;
    return 0;
}

// Cross-KV cache of all 12 layers in the attention kernel's operand format: built once per sampler call (or per denoise_step
// call) from the fp32 rank-5 tensors the C ABI hands over — 25 MB of traffic against 4 x 12 attention launches that then DMA it.
int Engine::pack_cross(hipStream_t st, Cond& c, int B, const CrossImg& carved) {
    c.img = CrossImg();
    if (!attn_img_ || (c.R <= 0 && c.P <= 0)) return 0;
    c.img = carved;
    const int pa = prec_[SITE_ATTN];
    CrossPackArgs p{};
    p.k_ref = c.k_ref; p.v_ref = c.v_ref; p.k_text = c.k_text; p.v_text = c.v_text;
    p.kc = carved.kc; p.kc_lo = img_lo(pa, carved.kc_lo); p.vtc = carved.vtc; p.vtc_lo = img_lo(pa, carved.vtc_lo);
    p.prec = pa; p.L = kBlocks; p.B = B; p.H = kHeads; p.dh = kDh; p.dhp = 128;
    p.R = c.R > 0 ? c.R : 0; p.P = c.P > 0 ? c.P : 0; p.Rp = carved.Rp; p.Cp = carved.Cp;
    ProfTag ptag("dit");
    HIPC(launch_cross_pack(p, st));
    return 0;
}

size_t Engine::denoise_ws_bytes(int B, int N, int R, int P, int rows) const { return dit_ws_bytes(B, N, R, P, rows, false, 0, 0); }

int Engine::denoise_step(hipStream_t st, const float* x_t, const uint8_t* mask, const float* t, const float* k_ref,
                         const float* v_ref, const uint8_t* ref_mask, const float* k_text, const float* v_text,
                         const uint8_t* ph_mask, const float* rope, int B, int N, int R, int P, float* velocity,
                         void* ws, size_t ws_bytes) {
    if (!dit_ready_) return fail("denoise_step: DiT weights not finalized");
    if (N > kMaxPos) return fail("denoise_step: sequence longer than the rope table (4096)");
    if (ws_bytes < denoise_ws_bytes(B, N, R, P, B)) return fail("denoise_step: workspace too small");
    if (ws_misaligned(ws)) return fail("denoise_step: workspace must be 256-byte aligned");
    HIPC(hipSetDevice(device_));
    DitWs w;
    w.plan(ws, B, N, R, P, B, false, 0, 0);
    if (modulation(st, t, B, w.m)) return 1;
    Cond cond{k_ref, v_ref, k_text, v_text, ref_mask, ph_mask, R, P, {}};
    if (pack_cross(st, cond, B, w.cross)) return 1;
    Call call(st);
    return denoise_core(st, x_t, mask, ModRow{w.m.mod, 0, 1, nullptr}, cond, rope, B, N, velocity, w.core, call);
}

// ---------------------------------------------------------------------------------------------
// S1 / S2 samplers
// ---------------------------------------------------------------------------------------------
void alpha_sigma_host(float t, float& a, float& s) {
    // reference infer/onnx.py:31-39 : float64 math on the float32 t, cast to float32 at the end
    double td = (double)t;
    const double eps = 1e-5;
    td = td < eps ? eps : (td > 1.0 - eps ? 1.0 - eps : td);
    double c = std::cos(M_PI / 2.0 * td);
    double a2 = c * c;
    double lsnr = std::log(a2 / (1.0 - a2)) + 2.0 * std::log(0.5);
    double asq = 1.0 / (1.0 + std::exp(-lsnr));
    a = (float)std::sqrt(asq);
    s = (float)std::sqrt(1.0 - asq);
}
static float linspace10(int i, int n) {
    // np.linspace(1, 0, n, dtype=float32): float64 arithmetic, endpoint exact, cast to float32
    if (n <= 1) return 1.0f;
    if (i == n - 1) return 0.0f;
    double step = -1.0 / (double)(n - 1);
    return (float)(1.0 + step * (double)i);
}

size_t Engine::sample_ws_bytes(int B, int N, int R, int P, int n_steps, int cfg) const {
    return dit_ws_bytes(B, N, R, P, n_steps, dit_fold_on((long)(cfg ? 3 * B : B) * N), n_steps, cfg);
}

int Engine::sample_pinned(hipStream_t st, int mode, int n_steps, int cfg, float s_text, float s_spk, const uint8_t* mask,
                          const float* k_ref, const float* v_ref, const uint8_t* ref_mask, const float* k_text,
                          const float* v_text, const uint8_t* ph_mask, int B, int N, int R, int P, const float* noise,
                          uint64_t seed, float* x_out, float* steps_out, void* ws, size_t ws_bytes, const uint8_t* sel_steps,
                          unsigned sel_layers, unsigned sel_heads, float* text_mass, const float* x_pin, const uint8_t* pin,
                          int start_step) {
    if (!dit_ready_) return fail("sample: DiT weights not finalized");
    if (n_steps < 1) return fail("sample: n_steps must be >= 1");
    if (N > kMaxPos) return fail("sample: sequence longer than the rope table (4096)");
    if (ws_bytes < sample_ws_bytes(B, N, R, P, n_steps, cfg)) return fail("sample: workspace too small");
    if (ws_misaligned(ws)) return fail("sample: workspace must be 256-byte aligned");
    // pinned frames (kernels.hip pin_renoise / pin_update): validated before anything is enqueued; without them nothing below differs
    const bool pinned = x_pin != nullptr || pin != nullptr || start_step != 0;
    if (pinned) {
        if (mode != 0) return fail("sample_pinned: pinned frames and start_step belong to mode 0 (the DMD sampler) only");
        if (cfg != 0) return fail("sample_pinned: pinned frames and start_step are not available with cfg");
        if (start_step < 0 || start_step >= n_steps) return fail("sample_pinned: start_step must lie in [0, n_steps)");
        if (start_step > 0 && !x_pin) return fail("sample_pinned: start_step > 0 starts from x_pin, which is NULL");
        if (pin && !x_pin) return fail("sample_pinned: pin needs x_pin");
        if ((((uintptr_t)x_pin | (uintptr_t)noise | (uintptr_t)ws) & 15) != 0)
            return fail("sample_pinned: x_pin, noise and the workspace must be 16-byte aligned");
    }
    // the text-attention tap (align.hip): validated before anything is enqueued; off (text_mass == null) nothing below differs from sample()
    Call call(st);
    AlignTap& tap = call.tap;
    std::vector<uint8_t> step_sel(n_steps, 0);
    if (text_mass) {
        if (!attn_img_) return fail("sample_align: the text-attention tap reads the attention operand images: not available with the image path switched off");
        if (B <= 0 || N <= 0 || P <= 0) return fail("sample_align: the tap needs frames and text keys (B, N, P > 0)");
        sel_layers &= (1u << kBlocks) - 1u;
        sel_heads &= (1u << kHeads) - 1u;
        int ns = 0, nl = 0, nh = 0;
        for (int i = start_step; i < n_steps; ++i) ns += (step_sel[i] = sel_steps ? (sel_steps[i] != 0) : (i + 1 == n_steps));
        for (int l = 0; l < kBlocks; ++l) nl += (sel_layers >> l) & 1u;
        for (int h = 0; h < kHeads; ++h) nh += (sel_heads >> h) & 1u;
        if (!ns || !nl || !nh) return fail("sample_align: the tap selects no (step, layer, head): 12 layers (bits 0..11), 8 heads (bits 0..7)");
        if (sizeof(float) * ((size_t)4 * (128 + pad8(N) + pad8(R > 0 ? R : 0) + pad8(P) + P) + 8) > 64 * 1024)
            return fail("sample_align: N + R + 2 P too large for the tap kernel's LDS tile");
        tap.mass = text_mass; tap.layers = sel_layers; tap.heads = sel_heads; tap.rows = B;
        tap.scale = 1.0f / (float)(ns * nl * nh);
    }
    HIPC(hipSetDevice(device_));
    const int Bd = cfg ? 3 * B : B;
    DitWs w;
    // (the fold replaces split-K partials + reduce; the 3B-row CFG batches of the teacher run unsplit + ln_modulate already, and there
    // the table kernel — every block weight once per four steps — and the heavier epilogue cost more than the norm launches: 239.0 vs
    // 240.6 ms per 128-step batch, profiles/r06l_ab_teacher_fold.txt)
    w.plan(ws, B, N, R, P, n_steps, dit_fold_on((long)Bd * N), n_steps, cfg);
    const SampleWs& s = w.s;
    const long e = (long)B * N * kLatent;

    std::vector<float> ts(n_steps), al(n_steps), sg(n_steps);
    for (int i = 0; i < n_steps; ++i) {
        ts[i] = linspace10(i, n_steps);
        alpha_sigma_host(ts[i], al[i], sg[i]);
    }
    // the same float32(np.linspace(1, 0, n)) values, generated on the device: a host -> device copy of the stack array would
    // need a stream synchronisation here, which drains the queue and leaves the GPU waiting on kernel launches for the
    // first DiT block of every batch (~0.1-0.5 ms of idle time in the rocprof timeline)
    HIPC(launch_linspace10(s.ts, n_steps, st));
    // t is shared by the whole batch -> every AdaLN vector of every step in one pass (SURVEY §7 hard part 3)
    // The table does not depend on the batch's data, only the first AdaLN needs it: in latency tuning it is computed on the
    // engine's side stream while the main stream packs the cross-KV images and embeds the first step's input (0.2 ms of tiny-M
    // GEMMs that fill a fraction of the chip); the main stream joins right before its first ln_modulate (denoise_core) — or, on an
    // early return between the fork and that point, when the call record goes (Call::~Call: ADVICE r3).
    if (dual_stream_ && !prof_on_) {
        if (!(call.side = side_set(st))) return 1;
        HIPC(hipEventRecord(call.side->fork, st));
        HIPC(hipStreamWaitEvent(call.side->stream, call.side->fork, 0));
        const int mod_rc = modulation(call.side->stream, s.ts, n_steps, w.m);
        HIPC(hipEventRecord(call.side->join, call.side->stream));   // recorded even when the chain failed half-way: what was enqueued is joined
        call.join_owed = true;
        if (mod_rc) return 1;
    } else if (modulation(st, s.ts, n_steps, w.m)) {
        return 1;
    }

    // the cross-KV cache in the attention kernel's operand format: once per call, read by every step
    Cond cond{k_ref, v_ref, k_text, v_text, ref_mask, ph_mask, R, P, {}};
    if (pack_cross(st, cond, Bd, w.cross)) return 1;
    // mask for 3B rows when cfg: caller passes mask with B rows; replicate by pointer arithmetic is impossible,
    // so the cfg path expects `mask` to already hold 3B rows (documented in the header).
    auto eval_velocity = [&](int step) -> int {
        tap.step_on = tap.mass && step_sel[step];
        const ModRow row{w.m.mod, step, 0, w.m.ftab};   // one row for the whole batch
        if (!cfg) return denoise_core(st, s.xt, mask, row, cond, nullptr, B, N, s.v, w.core, call);
        for (int r = 0; r < 3; ++r)
            HIPC(hipMemcpyAsync(s.xt3 + r * e, s.xt, e * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (denoise_core(st, s.xt3, mask, row, cond, nullptr, Bd, N, s.v3, w.core, call)) return 1;
        HIPC(launch_cfg_combine(s.v3, s.v, s_text, s_spk, e, st));
        return 0;
    };

    if (pinned) {
        // the same loop with the select in both element-wise steps; the first re-noise builds x itself (no memset, no launch more)
        for (int i = start_step; i < n_steps; ++i) {
            const float* nz = noise ? noise + (long)i * e : s.nz;
            if (!noise) HIPC(launch_randn(s.nz, e, seed, (uint64_t)i, st));   // always stream i, whatever start_step is
            HIPC(launch_pin_renoise(s.xt, s.x, x_pin, pin, mask, nz, al[i], sg[i], i > start_step ? 0 : start_step > 0 ? 2 : 1, e, st));
            if (eval_velocity(i)) return 1;
            HIPC(launch_pin_update(s.x, s.xt, s.v, x_pin, pin, mask, al[i], -sg[i], e, st));   // x = K ? x_pin : a x_t - s v
            if (steps_out) HIPC(hipMemcpyAsync(steps_out + (long)i * e, s.x, e * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    } else if (mode == 0) {
        HIPC(hipMemsetAsync(s.x, 0, e * sizeof(float), st));
        for (int i = 0; i < n_steps; ++i) {
            const float* nz = noise ? noise + (long)i * e : s.nz;
            if (!noise) HIPC(launch_randn(s.nz, e, seed, (uint64_t)i, st));
            HIPC(launch_axpby(s.xt, s.x, nz, al[i], sg[i], e, st));       // x_t = a x + s eps
            if (eval_velocity(i)) return 1;
            HIPC(launch_axpby(s.x, s.xt, s.v, al[i], -sg[i], e, st));     // x = a x_t - s v
            if (steps_out) HIPC(hipMemcpyAsync(steps_out + (long)i * e, s.x, e * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    } else {
        const float* nz = noise ? noise : s.nz;
        if (!noise) HIPC(launch_randn(s.nz, e, seed, 0, st));
        HIPC(hipMemsetAsync(s.x, 0, e * sizeof(float), st));
        HIPC(launch_axpby(s.xt, s.x, nz, 0.f, sg[0], e, st));             // x_1 = sigma(1) eps
        for (int i = 0; i < n_steps; ++i) {
            if (eval_velocity(i)) return 1;
            const bool last = i + 1 == n_steps;
            HIPC(launch_ode_step(s.xt, s.v, s.x, al[i], sg[i], last ? al[i] : al[i + 1], last ? sg[i] : sg[i + 1], e, st));
            if (steps_out) HIPC(hipMemcpyAsync(steps_out + (long)i * e, s.x, e * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    }
    HIPC(hipMemcpyAsync(x_out, s.x, e * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}
