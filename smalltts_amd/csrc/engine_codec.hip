// Engine, the codec: blocks and stage chain, plan and workspace, decode, streamed decode and encode.
#include "engine_impl.hpp"

// ---------------------------------------------------------------------------------------------
// Codec (V1 decode / V0 encode).  Channels-last images [B][kCodecPad + T][C]; the zero pad frames in
// front of each batch item implement the causal left padding of every conv, so strided / transposed /
// k-tap convs all become plain GEMMs over overlapping rows.
// ---------------------------------------------------------------------------------------------
// Stage chain (codec_ffn_wave.hip): every block of a C = 32 stage on each 32-frame tile back to back — the stage's image is read once
// and written once instead of once per block.  Returns 1 when the stage was enqueued (images swapped); 0 = not eligible, the
// caller runs the blocks one by one (bit-identical results either way: tests/test_codec_gpu.py::test_alternative_paths_*).
int Engine::codec_stage_chain(hipStream_t st, const CodecStageW& sg, float** xp, float** xaltp, int B, int T, int C) {
    const int F = cspec_.ffn_mult * C, nb = (int)sg.blocks.size();
    if (!stage_chain_ || !fused_ffn_ || !block_wave_ || nb < chain_min_blocks_ || nb > 3) return 0;
    int pf = prec_[SITE_CODEC_FFN];
    for (const CodecBlockW& b : sg.blocks) {
        if (pf == PREC_F16 && !b.f16_ok) return 0;   // an uncertified block runs split-bf16: per-block path
        if (b.w1.K != C || b.w2.K != F) return 0;
    }
    if (!codec_chain_wave_ok(C, F, cspec_.kernel, T, pf, nb)) return 0;
    {
        // Every wave of the chain walks ONE contiguous run of tiles plus a warm-up tile that is computed and not stored: with short runs
        // (small decodes: one 10 s utterance is 3 tiles per wave) the warm-up is a third of the work.  Measured (ADVICE r5,
        // profiles/r06q_chain_small_batch.txt, B x 10 s, chain vs one launch per block): B = 1 1.567 vs 1.554 ms, B = 4 (10 tiles per
        // wave) 3.538 vs 3.517, B = 8 (20) 5.923 vs 5.994 -> the chain from 16 tiles per wave up.
        const long waves = (long)(tune_.persist_cus > 0 ? tune_.persist_cus : num_cus_) * 12;
        if (chain_min_run_ > 0 && (long)B * T / 32 < chain_min_run_ * waves) return 0;
    }
    CodecChainBlock cb[3];
    for (int i = 0; i < nb; ++i) {
        const CodecBlockW& b = sg.blocks[i];
        cb[i] = CodecChainBlock{b.norm_w, b.dw_w, b.dw_b, b.gamma, b.ffn_norm_w, pf == PREC_F16 ? b.w1.h16 : b.w1.hi, b.w1.K, b.b1,
                                pf == PREC_F16 ? b.w2.h16 : b.w2.hi, b.b2, b.ffn_gamma};
    }
    const RowMap img = rowmap_batched(C, T, (long)(kCodecPad + T) * C, (long)kCodecPad * C);
    const hipError_t e = launch_codec_chain_wave(*xp, *xaltp, img, cb, nb, B * T, C, F, cspec_.kernel, cspec_.eps, pf, st, tune_);
    if (e != hipSuccess) { fail_hip(e, "codec stage chain"); return -1; }
    float* t = *xp; *xp = *xaltp; *xaltp = t;
    return 1;
}

int Engine::codec_block(hipStream_t st, const CodecBlockW& w, float** xp, float** xaltp, float* nbuf, bf16_t* n2hi,
                        bf16_t* n2lo, bf16_t* hhi, bf16_t* hlo, int B, int T, int C, size_t n2_elems, bool carried) {
    const int M = B * T, pad = kCodecPad;
    float* x = *xp;
    const RowMap img = rowmap_batched(C, T, (long)(pad + T) * C, (long)pad * C);
    const int F = cspec_.ffn_mult * C;
    const RowMap rc = rowmap_plain(C), rf = rowmap_plain(F);
    // a block whose fused-kernel range could not be certified never runs those kernels at fp16 (they do not clamp), whoever drives the C ABI
    const int pf = (prec_[SITE_CODEC_FFN] == PREC_F16 && !w.f16_ok) ? PREC_BF16X3 : prec_[SITE_CODEC_FFN];
    unsigned* const sf = satp(SITE_CODEC_FFN);
    bf16_t* const n2lo_f = sm_lo_for(pf, n2lo, sf);  // (hi, lo) pairs handed to producers: the format the FFN GEMMs read
    auto wsel = [pf](const PW& w) { return pf == PREC_F16 ? w.h16 : w.hi; };
    bool n2_done = false;  // the FFN's normalised input was already produced by the fused depthwise-conv kernel
    // narrowest stages: the whole block in one pass over the image (mixer + FFN, codec_ffn_wave.hip MIX kernels)
    if (fused_ffn_ && block_wave_ && codec_block_wave_ok(C, F, cspec_.kernel, T, pf) && w.w1.K == C && w.w2.K == F) {
        HIPC(launch_codec_block_wave(x, *xaltp, img, w.norm_w, w.dw_w, w.dw_b, w.gamma, w.ffn_norm_w, wsel(w.w1), w.w1.lo, w.w1.K, w.b1,
                                     wsel(w.w2), w.w2.lo, w.b2, w.ffn_gamma, M, C, F, cspec_.kernel, cspec_.eps, pf, st, tune_));
        *xp = *xaltp;
        *xaltp = x;
        return 0;
    }
    // mixer: RMSNorm -> causal depthwise conv -> LayerScale residual
    if (C <= 256 && 256 % (C / 4) == 0 && cspec_.kernel <= 7 && fused_ffn_) {  // narrow stages: one out-of-place kernel, then swap images
        HIPC(launch_mixer_fused(x, *xaltp, w.norm_w, w.dw_w, w.dw_b, w.gamma, B, T, C, cspec_.kernel, pad, cspec_.eps, st));
        *xp = *xaltp;
        *xaltp = x;
        x = *xp;
    } else if (fused_ffn_ && mixer_wide_ && mixer_wide_ok(C, cspec_.kernel) && F % 64 == 0 && (size_t)M * C <= n2_elems) {
        // wide stages: mixer + the FFN's RMSNorm in one out-of-place pass (no normalised fp32 image in between), then swap images
        HIPC(launch_mixer_wide(x, *xaltp, w.norm_w, w.dw_w, w.dw_b, w.gamma, w.ffn_norm_w, n2hi, n2lo_f, B, T, C, cspec_.kernel, pad,
                               cspec_.eps, st));
        *xp = *xaltp;
        *xaltp = x;
        x = *xp;
        n2_done = true;
    } else {
        HIPC(launch_rmsnorm(x, img, nbuf, nullptr, nullptr, img, M, C, cspec_.eps, w.norm_w, st));
        if (carried) {   // the conv reads K - 1 pad frames of the NORMALISED image: RMSNorm is per frame, so the carried frames' rows are exact
            const RowMap pm = rowmap_batched(C, pad, (long)(pad + T) * C, 0);
            HIPC(launch_rmsnorm(x, pm, nbuf, nullptr, nullptr, pm, B * pad, C, cspec_.eps, w.norm_w, st));
        }
        if (fused_ffn_ && C % 64 == 0 && F % 64 == 0 && C <= 2048) {  // + the FFN's RMSNorm of the updated rows (split pair n2)
            HIPC(launch_dwconv_resid_rms(x, nbuf, w.dw_w, w.dw_b, w.gamma, B, T, C, cspec_.kernel, pad, cspec_.eps, w.ffn_norm_w,
                                         n2hi, n2lo_f, rowmap_plain(C), st));
            n2_done = true;
        } else {
            HIPC(launch_dwconv_resid(x, nbuf, w.dw_w, w.dw_b, w.gamma, B, T, C, cspec_.kernel, pad, st));
        }
    }
    // FFN: RMSNorm -> Linear 4x -> GELU -> Linear -> LayerScale residual
    if (fused_ffn_ && (C == 32 || C == 64) && F == 4 * C && w.w1.K == C && w.w2.K == F) {
        // narrowest stages: all weights LDS-resident, one wave per 32 frames, hidden stays in registers (codec_ffn_wave.hip)
        HIPC(launch_codec_ffn_wave(x, img, w.ffn_norm_w, wsel(w.w1), w.w1.lo, w.w1.K, w.b1, wsel(w.w2), w.w2.lo, w.b2, w.ffn_gamma, M,
                                   C, F, cspec_.eps, pf, st, tune_));
        return 0;
    }
    if (w.w2t.N && fused_ffn_) {
        // C = 128 / 256: weights stream through an LDS ring, hidden in registers (codec_ffn_stream.hip)
        HIPC(launch_codec_ffn_stream(x, img, w.ffn_norm_w, wsel(w.w1), w.w1.lo, w.b1, wsel(w.w2t), w.w2t.lo, w.b2, w.ffn_gamma, M, C, F,
                                     cspec_.eps, pf, st, tune_));
        return 0;
    }
    // wide stages: two gemm3 launches; n2 / hidden are split bf16 pairs
    SplitBuf hid{hhi, hlo};
    if (F % 64 != 0) {  // hidden width not a whole k-tile (only tiny test specs): all-fp32-A path, hidden kept fp32
        float* hf = reinterpret_cast<float*>(hhi);  // hhi/hlo are adjacent: 2 x F x M bf16 = F x M fp32
        if (reinterpret_cast<char*>(hlo) < reinterpret_cast<char*>(hhi) + (size_t)M * F * 2) return fail("codec ws layout");
        HIPC(launch_rmsnorm(x, img, nbuf, nullptr, nullptr, img, M, C, cspec_.eps, w.ffn_norm_w, st));
        HIPC(gemm_store(ops(nbuf, img, w.w1, M), ACT_GELU, store_to(hf, rf, w.b1), 1, pf, st, tune_));
        EpiResid<0> r0{x, img, w.b2, w.ffn_gamma, 0, 0, 0, 1, nullptr};
        HIPC(gemm_resid(ops(hf, rf, w.w2, M), 2, r0, pf, st, tune_));
        return 0;
    }
    if (C % 64 == 0) {
        SplitBuf n2{n2hi, n2lo};
        if (!n2_done) HIPC(launch_rmsnorm(x, img, nullptr, n2hi, n2lo_f, rc, M, C, cspec_.eps, w.ffn_norm_w, st));
        HIPC(gemm3_store(ops3(n2, rc, w.w1, M, pf), ACT_GELU, store_split_to(hid.as(pf, sf), rf, w.b1), 1, pf, st, tune_));
    } else {  // K = C < 64 (last stage, C = 32): one k-tile on the fp32-A kernel, still writing the split hidden
        HIPC(launch_rmsnorm(x, img, nbuf, nullptr, nullptr, img, M, C, cspec_.eps, w.ffn_norm_w, st));
        HIPC(gemm_store(ops(nbuf, img, w.w1, M), ACT_GELU, store_split_to(hid.as(pf, sf), rf, w.b1), 1, pf, st, tune_));
    }
    EpiResid<0> r{x, img, w.b2, w.ffn_gamma, 0, 0, 0, 1, nullptr};
    {
        // M = 600 against a wide-K second product (the coarsest stage: 600 x 2048 x 8192): 160x128 tiles cut K so that ONE round
        // of workgroups fills the chip; fp32 partials go to the (now dead) n2 buffer, one pass reduces them in a fixed order
        // and applies bias / LayerScale / residual (same deterministic scheme as the DiT projections)
        const long t160 = (long)((M + 159) / 160) * ((C + 127) / 128);
        const int nk = F / 64;
        int splits = t160 > 0 && t160 <= 128 ? (int)(256 / t160) : 1;
        if (splits > nk / 8) splits = nk / 8;
        if (tune_.t160 && M > 480 && M <= 640 && splits >= 2 && (size_t)splits * M * C * 2 <= n2_elems && C % 4 == 0) {
            float* part = reinterpret_cast<float*>(n2hi);  // n2hi holds n2_elems bf16 = n2_elems / 2 floats
            HIPC(gemm3_resid_splitk(ops3(hid, rf, w.w2, M, pf), r, part, splits, pf, st, tune_, NextLN(), G3_160x128));
            return 0;
        }
    }
    {
        // fewer rows still (the codec ENCODER's coarse stages on 2-s references: 120 x 2048 x 8192 is 64 tiles that each walk the
        // whole K: 47 us at 0.7 TB/s of weights): K slices on 64x64 tiles + the same reduce
        const int splits = small_m_splitk_ && M <= 480 ? small_m_splits(M, F, 8, 1) : 1;
        if (splits >= 2 && fused_ffn_ && (size_t)splits * M * C * 2 <= n2_elems && C % 4 == 0) {
            float* part = reinterpret_cast<float*>(n2hi);
            HIPC(gemm3_resid_splitk(ops3(hid, rf, w.w2, M, pf), r, part, splits, pf, st, tune_, NextLN(), G3_64x64));
            return 0;
        }
    }
    HIPC(gemm3_resid(ops3(hid, rf, w.w2, M, pf), 2, r, pf, st, tune_));
    return 0;
}

Engine::CodecPlan Engine::codec_plan(bool decoder, int B, long T) const {
    // decoder: T latent frames; encoder: T audio samples
    const CodecSpecC& s = cspec_;
    const int S = s.n_ratios + 1;
    CodecPlan p;
    long Ti = T;
    for (int i = 0; i < S; ++i) {
        if (i > 0) Ti = decoder ? Ti * s.ratios[i - 1] : Ti / s.ratios[s.n_ratios - i];
        size_t C = (size_t)s.n_filters << (decoder ? S - 1 - i : i);
        size_t img = (size_t)B * (kCodecPad + Ti) * C;
        p.max_img = img > p.max_img ? img : p.max_img;
        size_t hid = (size_t)B * Ti * C * s.ffn_mult;
        p.max_hid = hid > p.max_hid ? hid : p.max_hid;
    }
    p.lat = decoder ? (size_t)B * (kCodecPad + T) * s.latent_dim : 1;
    return p;
}

size_t Engine::codec_ws_bytes(const CodecPlan& p) const {
    Bump b(nullptr);
    CodecWs w;
    w.plan(b, p);
    return b.off + 256;
}

size_t Engine::decode_ws_bytes(int B, int T) const { return codec_ws_bytes(codec_plan(true, B, T)); }

// latent image with causal zero pad, then stem conv k (as GEMM over K*latent contiguous floats) into w.xa; pads of the three
// images at the stage-0 geometry
int Engine::decode_stem(hipStream_t st, const CodecWs& w, const float* latents, int B, int T, const CodecCarry* cy) {
    const int pad = kCodecPad, Kc = cspec_.kernel, L = cspec_.latent_dim, C = dec_.stages[0].C;
    const int pcv = prec_[SITE_CODEC_CONV];
    const int pcv3 = pcv == PREC_F16 || pcv == PREC_F16X2 ? PREC_BF16X3 : pcv;  // the fp32-A kernel has no fp16 variant
    if (!cy) HIPC(launch_zero_pad_frames(w.lat, B, T, L, pad, st));
    HIPC(hipMemcpy2DAsync(w.lat + (long)pad * L, (size_t)(pad + T) * L * 4, latents, (size_t)T * L * 4, (size_t)T * L * 4, B,
                          hipMemcpyDeviceToDevice, st));
    if (cy) HIPC(cy->run(w.lat, B, T, L, cy->lay->lat, st));   // (behind the copy: the new state is the chunk's last frames)
    else HIPC(launch_zero_pad_frames3(w.xa, w.xb, w.nb, B, T, C, pad, st));
    RowMap am = rowmap_batched(L, T, (long)(pad + T) * L, (long)(pad - (Kc - 1)) * L);
    RowMap om = rowmap_batched(C, T, (long)(pad + T) * C, (long)pad * C);
    HIPC(gemm_store(ops(w.lat, am, dec_.stem, B * T), ACT_NONE, store_to(w.xa, om, dec_.stem_b), 1, pcv3, st, tune_));
    return 0;
}

// decoder stage i: the ConvTranspose into it (i > 0, what & 2), then its blocks (what & 4).  *x holds the image of (*Ti, *C) frames on
// entry and on return; *xn is the ping-pong partner
int Engine::decode_stage(hipStream_t st, const CodecWs& w, int i, int what, float** xp, float** xnp, int B, int* Tip, int* Cp,
                         const CodecCarry* cy) {
    static const char* kDecTags[] = {"dec.s0", "dec.s1", "dec.s2", "dec.s3", "dec.s4", "dec.s5", "dec.s6", "dec.s7"};
    ProfTag ptag(kDecTags[i < 8 ? i : 7]);
    const int pad = kCodecPad, pcv = prec_[SITE_CODEC_CONV];
    const int pcv3 = pcv == PREC_F16 || pcv == PREC_F16X2 ? PREC_BF16X3 : pcv;  // the fp32-A and streaming-upsample kernels have no fp16 variant
    const CodecStageW& sg = dec_.stages[i];
    float* x = *xp;
    float* xn = *xnp;
    int Ti = *Tip, C = *Cp;
    if (i > 0 && (what & 2)) {
        // ConvTranspose1d(k = 2r, stride r), causal trim: rows (x[t-1], x[t]) -> r output frames
        const int r = sg.r, Cn = sg.C, Tn = Ti * r;
        RowMap am = rowmap_batched(C, Ti, (long)(pad + Ti) * C, (long)(pad - 1) * C);
        RowMap om = rowmap_batched((long)r * Cn, Ti, (long)(pad + Tn) * Cn, (long)pad * Cn);
        if (cy) HIPC(cy->run(x, B, Ti, C, cy->lay->out[i - 1], st));   // frame t - 1 of the first output frames: the previous chunk's last
        if (fused_ffn_ && codec_upsample_wave_ok(sg.resample.K, sg.resample.N) && sg.resample.K == 2 * C && sg.resample.N == r * Cn)
            HIPC(launch_codec_upsample_wave(x, am, sg.resample.hi, sg.resample.lo, sg.resample.K, sg.resample_bias, xn, om,
                                            B * Ti, sg.resample.K, sg.resample.N, pcv3, st, tune_));
        else if (pcv == PREC_F16X2 && sg.resample.l16 && sg.resample.K % 64 == 0 && sg.resample.K >= x2_mink_ && sg.resample.K <= x2_maxk_ &&
                 C % 8 == 0 && (size_t)B * (pad + Ti) * C <= w.max_img) {
            // two-pass fp16 product: the image once as ONE fp16 array (pads included: the causal zeros), the weights as an fp16
            // hi + lo pair — A W_lo + A W_hi on the DMA-ring GEMM instead of three split-bf16 passes on the fp32-A kernel
            HIPC(launch_to_split(x, rowmap_plain(C), w.n2hi, sm_lo_for(PREC_F16, nullptr, satp(SITE_CODEC_CONV)), rowmap_plain(C), B * (pad + Ti), C, st));
            Gemm3Operands g3 = ops3(SplitBuf{w.n2hi, w.n2lo}, am, sg.resample, B * Ti, PREC_F16);
            g3.Wlo = sg.resample.l16;
            HIPC(gemm3_store_x2(g3, store_to(xn, om, sg.resample_bias), st, tune_));
        } else if (fused_ffn_ && sg.resample.K % 64 == 0 && sg.resample.K >= up_g3_mink_ && C % 8 == 0 && (size_t)B * (pad + Ti) * C <= w.max_img) {
            const int pg = pcv == PREC_F16X2 ? PREC_BF16X3 : pcv;   // (f16x2 outside its K range: split-bf16)
            // widest stages (K >= 2048; measured: 215 -> 148 us and 216 -> 193 us, no gain at K <= 1024): split the image once (pads included: they are the causal zeros) and run the DMA-ring GEMM on
            // the overlapping rows of the split pair (n2 is free between blocks)
            SplitBuf xs{w.n2hi, w.n2lo};
            HIPC(launch_to_split(x, rowmap_plain(C), xs.hi, xs.as(pg, satp(SITE_CODEC_CONV)).lo, rowmap_plain(C), B * (pad + Ti), C, st));
            HIPC(gemm3_store(ops3(xs, am, sg.resample, B * Ti, pg), ACT_NONE, store_to(xn, om, sg.resample_bias), 1, pg, st, tune_));
        } else
            HIPC(gemm_store(ops(x, am, sg.resample, B * Ti), ACT_NONE, store_to(xn, om, sg.resample_bias), 1, pcv3, st, tune_));
        float* t = x; x = xn; xn = t;
        Ti = Tn;
        C = Cn;
        // zero pads of the three images at the new geometry, in one launch BEHIND the product: it writes data rows only, and its
        // input (now the ping-pong partner) is free to be overwritten from here on
        if (!cy) HIPC(launch_zero_pad_frames3(x, xn, w.nb, B, Ti, C, pad, st));
    }
    *Tip = Ti;
    *Cp = C;
    if ((what & 4) && cy) {
        // the images ping-pong and out-of-place kernels write no pad frames: the carry goes on the current input in front of EVERY block
        for (size_t j = 0; j < sg.blocks.size(); ++j) {
            HIPC(cy->run(x, B, Ti, C, cy->lay->block[i][j], st));
            if (codec_block(st, sg.blocks[j], &x, &xn, w.nb, w.n2hi, w.n2lo, w.hhi, w.hlo, B, Ti, C, w.max_img, true)) return 1;
        }
    } else if (what & 4) {
        if (const int ch = codec_stage_chain(st, sg, &x, &xn, B, Ti, C)) {   // > 0: the whole stage went out as one launch
            if (ch < 0) return 1;
        } else {
            for (const CodecBlockW& b : sg.blocks)
                if (codec_block(st, b, &x, &xn, w.nb, w.n2hi, w.n2lo, w.hhi, w.hlo, B, Ti, C, w.max_img)) return 1;
        }
    }
    *xp = x;
    *xnp = xn;
    return 0;
}

// final RMSNorm (if loaded) + head conv: the image of the last stage -> (B, Ti) audio
int Engine::decode_head(hipStream_t st, const CodecWs& w, float* x, int B, int Ti, int C, float* audio, const CodecCarry* cy) {
    const int pad = kCodecPad;
    if (cy) HIPC(cy->run(x, B, Ti, C, cy->lay->head, st));
    if (dec_.final_norm_w) {   // out of place into the (zero-padded) scratch image: the head conv reads K - 1 pad frames
        const RowMap img = rowmap_batched(C, Ti, (long)(pad + Ti) * C, (long)pad * C);
        HIPC(launch_rmsnorm(x, img, w.nb, nullptr, nullptr, img, B * Ti, C, cspec_.eps, dec_.final_norm_w, st));
        if (cy) {   // ... which here hold the carried frames, normalised like every other frame
            const RowMap pm = rowmap_batched(C, pad, (long)(pad + Ti) * C, 0);
            HIPC(launch_rmsnorm(x, pm, w.nb, nullptr, nullptr, pm, B * pad, C, cspec_.eps, dec_.final_norm_w, st));
        }
        x = w.nb;
    }
    HIPC(launch_head_conv(x, dec_.head_w, dec_.head_b_host, audio, B, Ti, C, cspec_.kernel, pad, st));
    return 0;
}

int Engine::codec_decode(hipStream_t st, const float* latents, int B, int T, float* audio, void* ws, size_t ws_bytes) {
    if (!dec_.ready) return fail("codec_decode: decoder weights not finalized");
    const CodecPlan plan = codec_plan(true, B, T);
    if (ws_bytes < codec_ws_bytes(plan)) return fail("codec_decode: workspace too small");
    if (ws_misaligned(ws)) return fail("codec_decode: workspace must be 256-byte aligned");
    HIPC(hipSetDevice(device_));
    Bump bump(ws);
    CodecWs w;
    w.plan(bump, plan);
    if (decode_stem(st, w, latents, B, T)) return 1;
    float* x = w.xa;
    float* xn = w.xb;
    int Ti = T, C = dec_.stages[0].C;
    for (int i = 0; i < cspec_.n_ratios + 1; ++i)
        if (decode_stage(st, w, i, 2 | 4, &x, &xn, B, &Ti, &C)) return 1;
    return decode_head(st, w, x, B, Ti, C, audio);
}

// ---- streamed decode --------------------------------------------------------------------------------------------------------------
Engine::DecodeStateLayout Engine::decode_state_layout() const {
    const CodecSpecC& s = cspec_;
    const int S = s.n_ratios + 1;
    DecodeStateLayout l;
    size_t off = 0;
    auto take = [&](size_t C) { const size_t o = off; off += (size_t)kCodecPad * C * sizeof(float); ++l.count; return o; };
    auto width = [&](int i) { return (size_t)s.n_filters << (S - 1 - i); };
    l.lat = take((size_t)s.latent_dim);
    l.block.resize(S);
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < s.depths[i]; ++j) l.block[i].push_back(take(width(i)));
    for (int i = 0; i + 1 < S; ++i) l.out.push_back(take(width(i)));
    l.head = take(width(S - 1));
    l.bytes = (off + 255) & ~size_t(255);
    return l;
}

int Engine::codec_decode_stream(hipStream_t st, const float* latents, int B, int T, void* pool, int64_t n_slots, const int64_t* slots,
                                float* audio, void* ws, size_t ws_bytes) {
    if (!dec_.ready) return fail("codec_decode_stream: decoder weights not finalized");
    if (B < 1 || T < 1) return fail("codec_decode_stream: B and T must be positive");
    if (!latents || !pool || !slots || !audio) return fail("codec_decode_stream: a required pointer is NULL");
    if (n_slots < 1) return fail("codec_decode_stream: the state pool has no slots");
    if (reinterpret_cast<uintptr_t>(pool) & 15) return fail("codec_decode_stream: the state pool must be 16-byte aligned");
    if ((cspec_.latent_dim | cspec_.n_filters) % 4) return fail("codec_decode_stream: channel counts must be multiples of 4");
    const CodecPlan plan = codec_plan(true, B, T);
    if (ws_bytes < codec_ws_bytes(plan)) return fail("codec_decode_stream: workspace too small");
    if (ws_misaligned(ws)) return fail("codec_decode_stream: workspace must be 256-byte aligned");
    const DecodeStateLayout lay = decode_state_layout();
    for (size_t i = 0; i < lay.block.size(); ++i)
        if (lay.block[i].size() != dec_.stages[i].blocks.size()) return fail("codec_decode_stream: the codec spec changed after finalize");
    HIPC(hipSetDevice(device_));
    const CodecCarry cy{pool, (long)lay.bytes, (long)n_slots, slots, &lay};
    Bump bump(ws);
    CodecWs w;
    w.plan(bump, plan);
    if (decode_stem(st, w, latents, B, T, &cy)) return 1;
    float* x = w.xa;
    float* xn = w.xb;
    int Ti = T, C = dec_.stages[0].C;
    for (int i = 0; i < cspec_.n_ratios + 1; ++i)
        if (decode_stage(st, w, i, 2 | 4, &x, &xn, B, &Ti, &C, &cy)) return 1;
    return decode_head(st, w, x, B, Ti, C, audio, &cy);
}

size_t Engine::encode_ws_bytes(int B, int S_) const { return codec_ws_bytes(codec_plan(false, B, S_)); }

// The coarse end of the encoder on short references is a handful of rows against a long K (2-s references: the last strided
// conv is 120 x 2048 x 16384, the head 120 x 64 x 14336): as row tiles alone that is 2-32 workgroups streaming 134 MB of
// weights (374 / 254 us).  There: convert the (small) image once to the GEMM operand format — pads included, they are the
// causal zeros — and run gemm3 over the overlapping rows as K slices + one reduce.  Returns 1 when it took the product, 0 when
// the caller runs it, -1 on a launch error.
int Engine::conv_small_m(hipStream_t st, const CodecWs& w, const float* img, long img_rows, int Cin, const RowMap& am, const PW& wt,
                         const float* bias, float* out, const RowMap& om, int M) {
    const int pcv = prec_[SITE_CODEC_CONV];
    const int splits = (small_m_splitk_ && fused_ffn_ && wt.K >= 2048) ? small_m_splits(M, wt.K, 8, 4) : 1;
    if (splits < 2 || wt.K % 64 || Cin % 4 || wt.N % 4 || (size_t)img_rows * Cin > w.max_img || (size_t)splits * M * wt.N * 2 > w.max_hid)
        return 0;
    SplitBuf xs{w.n2hi, w.n2lo};
    float* part = reinterpret_cast<float*>(w.hhi);   // max_hid bf16 = max_hid / 2 floats
    hipError_t e = launch_to_split(img, rowmap_plain(Cin), xs.hi, xs.as(pcv, satp(SITE_CODEC_CONV)).lo, rowmap_plain(Cin), (int)img_rows, Cin, st);
    if (e == hipSuccess) e = gemm3_store_splitk(ops3(xs, am, wt, M, pcv), part, splits, pcv, bias, out, om, st, tune_);
    if (e != hipSuccess) { fail_hip(e, "codec_encode: split-K conv"); return -1; }
    return 1;
}

// encoder stem: (B, S) audio -> the stage-0 image in w.xa; pads of the three images at the stage-0 geometry
int Engine::encode_stem(hipStream_t st, const CodecWs& w, const float* audio, int B, int S_) {
    const int C = enc_.stages[0].C;
    HIPC(launch_zero_pad_frames3(w.xa, w.xb, w.nb, B, S_, C, kCodecPad, st));
    HIPC(launch_stem_conv1(audio, enc_.stem_w_raw, enc_.stem_b, w.xa, B, S_, C, cspec_.kernel, kCodecPad, st));
    return 0;
}

// encoder stage i: the strided conv into it (i > 0, what & 2), then its blocks (what & 4); arguments as decode_stage
int Engine::encode_stage(hipStream_t st, const CodecWs& w, int i, int what, float** xp, float** xnp, int B, int* Tip, int* Cp) {
    static const char* kEncTags[] = {"cenc.s0", "cenc.s1", "cenc.s2", "cenc.s3", "cenc.s4", "cenc.s5", "cenc.s6", "cenc.s7"};
    ProfTag ptag(kEncTags[i < 8 ? i : 7]);
    const int pad = kCodecPad;
    const int pcv3 = prec_[SITE_CODEC_CONV] == PREC_F16 || prec_[SITE_CODEC_CONV] == PREC_F16X2 ? PREC_BF16X3 : prec_[SITE_CODEC_CONV];
    const CodecStageW& sg = enc_.stages[i];
    float* x = *xp;
    float* xn = *xnp;
    int Ti = *Tip, C = *Cp;
    if (i > 0 && (what & 2)) {
        // Conv1d(k = 2r, stride r), causal left pad r: out[t] reads frames [(t-1) r, (t+1) r)
        const int r = sg.r, Cn = sg.C, Tn = Ti / r;
        RowMap am = rowmap_batched((long)r * C, Tn, (long)(pad + Ti) * C, (long)(pad - r) * C);
        RowMap om = rowmap_batched(Cn, Tn, (long)(pad + Tn) * Cn, (long)pad * Cn);
        const int took = conv_small_m(st, w, x, (long)B * (pad + Ti), C, am, sg.resample, sg.resample_bias, xn, om, B * Tn);
        if (took < 0) return 1;
        if (!took) HIPC(gemm_store(ops(x, am, sg.resample, B * Tn), ACT_NONE, store_to(xn, om, sg.resample_bias), 1, pcv3, st, tune_));
        float* t = x; x = xn; xn = t;
        Ti = Tn;
        C = Cn;
        HIPC(launch_zero_pad_frames3(x, xn, w.nb, B, Ti, C, pad, st));   // (behind the product, as in the decoder)
    }
    *Tip = Ti;
    *Cp = C;
    if (what & 4) {
        if (const int ch = codec_stage_chain(st, sg, &x, &xn, B, Ti, C)) {
            if (ch < 0) return 1;
        } else {
            for (const CodecBlockW& b : sg.blocks)
                if (codec_block(st, b, &x, &xn, w.nb, w.n2hi, w.n2lo, w.hhi, w.hlo, B, Ti, C, w.max_img)) return 1;
        }
    }
    *xp = x;
    *xnp = xn;
    return 0;
}

// final RMSNorm (if loaded) + head conv: the image of the last stage -> (B, Ti, latent)
int Engine::encode_head(hipStream_t st, const CodecWs& w, const float* x, int B, int Ti, int C, float* latents) {
    const int pad = kCodecPad, Kc = cspec_.kernel;
    const int pcv3 = prec_[SITE_CODEC_CONV] == PREC_F16 || prec_[SITE_CODEC_CONV] == PREC_F16X2 ? PREC_BF16X3 : prec_[SITE_CODEC_CONV];
    if (enc_.final_norm_w) {
        const RowMap img = rowmap_batched(C, Ti, (long)(pad + Ti) * C, (long)pad * C);
        HIPC(launch_rmsnorm(x, img, w.nb, nullptr, nullptr, img, B * Ti, C, cspec_.eps, enc_.final_norm_w, st));
        x = w.nb;
    }
    RowMap am = rowmap_batched(C, Ti, (long)(pad + Ti) * C, (long)(pad - (Kc - 1)) * C);
    const int took = conv_small_m(st, w, x, (long)B * (pad + Ti), C, am, enc_.head, enc_.head_b, latents, rowmap_plain(cspec_.latent_dim), B * Ti);
    if (took < 0) return 1;
    if (!took)
        HIPC(gemm_store(ops(x, am, enc_.head, B * Ti), ACT_NONE, store_to(latents, rowmap_plain(cspec_.latent_dim), enc_.head_b), 1,
                        pcv3, st, tune_));
    return 0;
}

int Engine::codec_encode(hipStream_t st, const float* audio, int B, int S_, float* latents, void* ws, size_t ws_bytes) {
    if (!enc_.ready) return fail("codec_encode: encoder weights not finalized");
    const CodecPlan plan = codec_plan(false, B, S_);
    if (ws_bytes < codec_ws_bytes(plan)) return fail("codec_encode: workspace too small");
    if (ws_misaligned(ws)) return fail("codec_encode: workspace must be 256-byte aligned");
    HIPC(hipSetDevice(device_));
    Bump bump(ws);
    CodecWs w;
    w.plan(bump, plan);
    if (encode_stem(st, w, audio, B, S_)) return 1;
    float* x = w.xa;
    float* xn = w.xb;
    int Ti = S_, C = enc_.stages[0].C;
    for (int i = 0; i < cspec_.n_ratios + 1; ++i)
        if (encode_stage(st, w, i, 2 | 4, &x, &xn, B, &Ti, &C)) return 1;
    return encode_head(st, w, x, B, Ti, C, latents);
}
