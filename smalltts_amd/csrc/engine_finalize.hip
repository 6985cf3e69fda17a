// Engine, finalize: the packs the DiT, the condition encoders and the codec read, built from the registered tensors.
#include "engine_impl.hpp"

std::vector<int> swiglu_perm(int F) {
    std::vector<int> p(2 * F);
    for (int i = 0; i < 2 * F; ++i) {
        int blk = i / 64, within = i % 64;
        p[i] = within < 32 ? blk * 32 + within : F + blk * 32 + (within - 32);
    }
    return p;
}

int Engine::build_encoder(EncoderW& e, const std::string& prefix, int dim, int heads, int ff, int layers, float eps) {
    e.dim = dim; e.heads = heads; e.dh = dim / heads; e.ff = ff; e.layers = layers; e.eps = eps;
    if (ff % 32) return fail("encoder ff must be a multiple of 32");
    std::vector<int> perm = swiglu_perm(ff);
    e.blocks.clear();
    for (int i = 0; i < layers; ++i) {
        std::string p = sidx(prefix + ".blocks.", i, "");
        for (const char* n : {"wq", "wk", "wv", "wo", "gate"})
            if (check_shape(p + ".attention." + n + ".weight", {dim, dim})) return 1;
        if (check_shape(p + ".attention.q_norm.weight", {heads, dim / heads}) || check_shape(p + ".attention.k_norm.weight", {heads, dim / heads}) ||
            check_shape(p + ".mlp.w1.weight", {ff, dim}) || check_shape(p + ".mlp.w3.weight", {ff, dim}) ||
            check_shape(p + ".mlp.w2.weight", {dim, ff}) || check_shape(p + ".attention_norm.weight", {dim}) ||
            check_shape(p + ".mlp_norm.weight", {dim}))
            return 1;
        EncBlockW b;
        b.qkvg = pack_rows({p + ".attention.wq.weight", p + ".attention.wk.weight", p + ".attention.wv.weight",
                            p + ".attention.gate.weight"});
        b.wo = pack_rows({p + ".attention.wo.weight"});
        b.ff13 = pack_rows({p + ".mlp.w1.weight", p + ".mlp.w3.weight"}, &perm);
        b.w2 = pack_rows({p + ".mlp.w2.weight"});
        b.qn = rawp(p + ".attention.q_norm.weight");
        b.kn = rawp(p + ".attention.k_norm.weight");
        b.an = rawp(p + ".attention_norm.weight");
        b.mn = rawp(p + ".mlp_norm.weight");
        if (!b.qkvg.N || !b.wo.N || !b.ff13.N || !b.w2.N || !b.qn || !b.kn || !b.an || !b.mn)
            return fail("encoder block incomplete: " + p + " (" + err_ + ")");
        e.blocks.push_back(b);
    }
    e.final_norm = rawp(prefix + ".norm.weight");
    if (!e.final_norm) return fail("missing " + prefix + ".norm.weight");
    return make_rope(e.dh, &e.rope_cos, &e.rope_sin);
}

int Engine::make_rope(int dim, float** cos_out, float** sin_out) {
    const size_t n = (size_t)kMaxPos * dim;
    float* ang = nullptr;
    HIPC(hipMalloc(&ang, n * 4));
    *cos_out = static_cast<float*>(dalloc(n * 4));
    *sin_out = static_cast<float*>(dalloc(n * 4));
    if (!*cos_out || !*sin_out) return fail("rope table alloc failed");
    HIPC(launch_rope_table(ang, kMaxPos, dim, 0));
    HIPC(launch_rope_cossin(ang, *cos_out, *sin_out, (int)n, 0));
    HIPC(hipStreamSynchronize(0));
    HIPC(hipFree(ang));
    return 0;
}

int Engine::finalize_dit() {
    const std::string T = "dit.transformer_blocks.";
    // shape contract of DiTModel(64).state_dict() (reference model.py:33-54): the kernels assume these strides, so a checkpoint
    // of another model size must fail here with the tensor's name instead of reading out of bounds later
    {
        const long H = kHidden, FF = kFF;
        struct { const char* n; std::initializer_list<long> sh; } g[] = {
            {"time_embedding.mlp.0.weight", {H, 256}}, {"time_embedding.mlp.0.bias", {H}},
            {"time_embedding.mlp.2.weight", {H, H}}, {"time_embedding.mlp.2.bias", {H}},
            {"dit.emb_proj.0.weight", {2 * H, H}}, {"dit.emb_proj.0.bias", {2 * H}},
            {"dit.emb_proj.2.weight", {H, 2 * H}}, {"dit.emb_proj.2.bias", {H}},
            {"dit.input_embed.proj.weight", {H, kLatent}}, {"dit.input_embed.proj.bias", {H}},
            {"dit.input_embed.conv_pos_embed.conv1.bias", {H}}, {"dit.input_embed.conv_pos_embed.conv2.bias", {H}},
            {"dit.phoneme_proj.weight", {H, 512}}, {"dit.phoneme_proj.bias", {H}},
            {"dit.norm_out.linear.weight", {2 * H, H}}, {"dit.norm_out.linear.bias", {2 * H}},
            {"velocity.weight", {kLatent, H}}, {"velocity.bias", {kLatent}},
            {"style_encoder.in_proj.weight", {512, kLatent}}, {"style_encoder.in_proj.bias", {512}},
            {"style_encoder.out_proj.weight", {H, 512}}, {"style_encoder.out_proj.bias", {H}},
            {"style_encoder.log_scale", {}}, {"phoneme_embedding.text_embedding.weight", {198, 512}},
        };
        for (auto& t : g)
            if (check_shape(t.n, t.sh)) return 1;
        for (int i = 0; i < kBlocks; ++i) {
            const std::string p = sidx(T, i, "");
            for (const char* n : {"to_q", "to_k_self", "to_v_self", "to_k_ref", "to_v_ref", "to_k_text", "to_v_text"})
                if (check_shape(p + ".attn." + n + ".weight", {H, H}) || check_shape(p + ".attn." + n + ".bias", {H})) return 1;
            if (check_shape(p + ".attn.gate.weight", {H, H}) || check_shape(p + ".attn.to_out.0.weight", {H, H})) return 1;
            for (const char* n : {"q_norm", "k_norm", "k_norm_cross"})
                if (check_shape(p + ".attn." + n + ".weight", {kHeads, kDh})) return 1;
            if (check_shape(p + ".attn_norm.linear.weight", {6 * H, H}) || check_shape(p + ".attn_norm.linear.bias", {6 * H})) return 1;
            if (check_shape(p + ".ff.w1.weight", {FF, H}) || check_shape(p + ".ff.w1.bias", {FF}) ||
                check_shape(p + ".ff.w3.weight", {FF, H}) || check_shape(p + ".ff.w3.bias", {FF}) ||
                check_shape(p + ".ff.w2.weight", {H, FF}) || check_shape(p + ".ff.w2.bias", {H}))
                return 1;
        }
    }
    time0_ = pack_rows({"time_embedding.mlp.0.weight"});
    time2_ = pack_rows({"time_embedding.mlp.2.weight"});
    emb0_ = pack_rows({"dit.emb_proj.0.weight"});
    emb2_ = pack_rows({"dit.emb_proj.2.weight"});
    inproj_ = pack_rows({"dit.input_embed.proj.weight"});
    velocity_ = pack_rows({"velocity.weight"});
    phproj_ = pack_rows({"dit.phoneme_proj.weight"});
    style_in_ = pack_rows({"style_encoder.in_proj.weight"});
    style_out_ = pack_rows({"style_encoder.out_proj.weight"});
    if (!time0_.N || !time2_.N || !emb0_.N || !emb2_.N || !inproj_.N || !velocity_.N || !phproj_.N || !style_in_.N ||
        !style_out_.N)
        return fail("DiT pack failed: " + err_);

    std::vector<std::string> modw, modb, kvr, kvrb, kvt, kvtb, knc;
    for (int i = 0; i < kBlocks; ++i) {
        std::string p = sidx(T, i, "");
        modw.push_back(p + ".attn_norm.linear.weight");
        modb.push_back(p + ".attn_norm.linear.bias");
        kvr.push_back(p + ".attn.to_k_ref.weight"); kvr.push_back(p + ".attn.to_v_ref.weight");
        kvrb.push_back(p + ".attn.to_k_ref.bias"); kvrb.push_back(p + ".attn.to_v_ref.bias");
        kvt.push_back(p + ".attn.to_k_text.weight"); kvt.push_back(p + ".attn.to_v_text.weight");
        kvtb.push_back(p + ".attn.to_k_text.bias"); kvtb.push_back(p + ".attn.to_v_text.bias");
        knc.push_back(p + ".attn.k_norm_cross.weight");
    }
    modw.push_back("dit.norm_out.linear.weight");
    modb.push_back("dit.norm_out.linear.bias");
    modall_ = pack_rows(modw);
    modall_b_ = concat_vec(modb);
    kvref_ = pack_rows(kvr);
    kvref_b_ = concat_vec(kvrb);
    kvtext_ = pack_rows(kvt);
    kvtext_b_ = concat_vec(kvtb);
    knc_ = concat_vec(knc);
    if (!modall_.N || !modall_b_ || !kvref_.N || !kvref_b_ || !kvtext_.N || !kvtext_b_ || !knc_)
        return fail("DiT modulation/KV pack failed: " + err_);
    if (modall_.N != kModLd) return fail("modulation table width mismatch");

    // grouped conv (dit.py:218-220) -> per-group GEMM weights [G*cpg][K*64] (ic padded 60 -> 64)
    for (int c = 0; c < 2; ++c) {
        const RawTensor* w = raw(sidx("dit.input_embed.conv_pos_embed.conv", c + 1, ".weight"));
        if (!w || w->shape.size() != 3 || w->shape[0] != kHidden || w->shape[1] != kConvCpg || w->shape[2] != kConvK)
            return fail("conv_pos_embed weight missing or wrong shape");
        float* tmp = nullptr;
        const int Kp = kConvK * kConvGs;
        HIPC(hipMalloc(&tmp, (size_t)kHidden * Kp * 4));
        GatherSpec g{0, 0, (long)kConvCpg * kConvK, 1, kConvK, kHidden, kConvGs, kConvCpg};
        HIPC(launch_gather_pack(w->d, tmp, kHidden, Kp, g, 0));
        (c ? conv2_ : conv1_) = pack_from_f32(tmp, kHidden, Kp);
        HIPC(hipStreamSynchronize(0));
        HIPC(hipFree(tmp));
        if (!(c ? conv2_ : conv1_).N) return fail("conv pack failed");
    }

    std::vector<int> perm = swiglu_perm(kFF);
    std::vector<int> hperm(4 * kHeads * 128, -1);   // row (part * 8 + h) * 128 + d <- source row part * 960 + h * 120 + d, pad rows zero
    for (int part = 0; part < 4; ++part)
        for (int h = 0; h < kHeads; ++h)
            for (int d = 0; d < kDh; ++d) hperm[(part * kHeads + h) * 128 + d] = part * kHidden + h * kDh + d;
    blocks_.clear();
    qkvg_unpadded_ready_ = false;
    for (int i = 0; i < kBlocks; ++i) {
        std::string p = sidx(T, i, "");
        DitBlockW b;
        b.name = p;
        if (!(attn_img_ && attn_epi_))   // (the default path reads the head-padded pack only: ensure_qkvg_unpadded builds this one on demand)
            b.qkvg = pack_rows({p + ".attn.to_q.weight", p + ".attn.to_k_self.weight", p + ".attn.to_v_self.weight",
                                p + ".attn.gate.weight"});
        b.b_qkvg = concat_vec({p + ".attn.to_q.bias", p + ".attn.to_k_self.bias", p + ".attn.to_v_self.bias", ""},
                              {kHidden});
        b.qkvgp = pack_rows({p + ".attn.to_q.weight", p + ".attn.to_k_self.weight", p + ".attn.to_v_self.weight",
                             p + ".attn.gate.weight"}, &hperm);
        b.b_qkvgp = static_cast<float*>(dalloc(hperm.size() * 4));
        if (b.b_qkvgp && b.b_qkvg) {   // the padded bias: gather on the host side of a tiny vector
            std::vector<float> src(4 * kHidden), dst(hperm.size(), 0.f);
            (void)hipMemcpy(src.data(), b.b_qkvg, src.size() * 4, hipMemcpyDeviceToHost);
            for (size_t r = 0; r < hperm.size(); ++r) if (hperm[r] >= 0) dst[r] = src[hperm[r]];
            (void)hipMemcpy(b.b_qkvgp, dst.data(), dst.size() * 4, hipMemcpyHostToDevice);
        }
        b.out = pack_rows({p + ".attn.to_out.0.weight"});
        b.ff13 = pack_rows({p + ".ff.w1.weight", p + ".ff.w3.weight"}, &perm);
        b.ff2 = pack_rows({p + ".ff.w2.weight"}, nullptr, kFFp);
        b.b1 = rawp(p + ".ff.w1.bias"); b.b3 = rawp(p + ".ff.w3.bias"); b.b2 = rawp(p + ".ff.w2.bias");
        b.qn = rawp(p + ".attn.q_norm.weight"); b.kn = rawp(p + ".attn.k_norm.weight");
        if ((!(attn_img_ && attn_epi_) && !b.qkvg.N) || !b.qkvgp.N || !b.b_qkvg || !b.b_qkvgp || !b.out.N || !b.ff13.N || !b.ff2.N || !b.b1 || !b.b3 || !b.b2 || !b.qn || !b.kn)
            return fail("DiT block incomplete: " + p + " (" + err_ + ")");
        blocks_.push_back(b);
    }
    if (build_encoder(style_, "style_encoder", 512, 8, 1536, 12, 1e-5f)) return 1;
    if (build_encoder(text_, "phoneme_embedding", 512, 4, 1024, 8, 1e-6f)) return 1;
    float ls = 0.f;
    if (!raw("style_encoder.log_scale")) return fail("missing style_encoder.log_scale");
    HIPC(hipMemcpy(&ls, rawp("style_encoder.log_scale"), 4, hipMemcpyDeviceToHost));
    style_scale_ = expf(ls);
    if (make_rope(64, &rope_dit_cos_, &rope_dit_sin_)) return 1;
    for (const char* n : {"time_embedding.mlp.0.bias", "time_embedding.mlp.2.bias", "dit.emb_proj.0.bias",
                          "dit.emb_proj.2.bias", "dit.input_embed.proj.bias", "velocity.bias", "dit.phoneme_proj.bias",
                          "style_encoder.in_proj.bias", "style_encoder.out_proj.bias",
                          "dit.input_embed.conv_pos_embed.conv1.bias", "dit.input_embed.conv_pos_embed.conv2.bias",
                          "phoneme_embedding.text_embedding.weight"})
        if (!raw(n)) return fail(std::string("missing tensor ") + n);
    dit_ready_ = true;
    return 0;
}

int Engine::finalize_codec(bool decoder) {
    const CodecSpecC& s = cspec_;
    CodecHalfW& h = decoder ? dec_ : enc_;
    const std::string P = decoder ? "codec.decoder" : "codec.encoder";
    const int S = s.n_ratios + 1, Kc = s.kernel;
    if (Kc - 1 > kCodecPad) return fail("codec kernel too large for the frame padding");
    h = CodecHalfW();
    // Optional tensors (CodecSpec flags conv_bias / ffn_bias / layer_scale, smalltts_amd/weights.py): an exported codec may come
    // without biases or layer scales — absent means the identity value, present means the inventory's shape.
    auto opt_vec = [&](const std::string& name, long n, float fill, const float** out) -> int {
        if (raw(name)) {
            if (check_shape(name, {n})) return 1;
            *out = rawp(name);
            return 0;
        }
        float* d = static_cast<float*>(dalloc((size_t)n * 4));
        if (!d) return fail("codec: out of memory for the default of " + name);
        HIPC(launch_fill(d, fill, n, 0));
        *out = d;
        return 0;
    };
    auto gather_to_pw = [&](const float* src, int N, int K, GatherSpec g, PW& out, float** f32_out, bool x2 = false) -> int {
        float* tmp = nullptr;
        if (f32_out) {
            tmp = static_cast<float*>(dalloc((size_t)N * K * 4));
            if (!tmp) return fail("codec pack alloc failed");
        } else {
            HIPC(hipMalloc(&tmp, (size_t)N * K * 4));
        }
        HIPC(launch_gather_pack(src, tmp, N, K, g, 0));
        if (f32_out) { *f32_out = tmp; return 0; }
        out = pack_from_f32(tmp, N, K);
        if (x2 && out.N) {   // low half of the fp16 pair (PREC_F16X2)
            out.l16 = static_cast<bf16_t*>(dalloc((size_t)N * K * 2));
            if (!out.l16) return fail("codec pack alloc failed");
            HIPC(launch_f16_residual(tmp, K, out.h16, out.l16, out.K, N, K, 0));
        }
        HIPC(hipStreamSynchronize(0));
        HIPC(hipFree(tmp));
        return out.N ? 0 : fail("codec pack failed");
    };
    for (int i = 0; i < S; ++i) {
        CodecStageW st;
        const int C = decoder ? s.n_filters << (S - 1 - i) : s.n_filters << i;
        st.C = C;
        if (i > 0) {
            const int r = decoder ? s.ratios[i - 1] : s.ratios[s.n_ratios - i];
            if (r > kCodecPad) return fail("codec ratio exceeds frame padding");
            st.r = r;
            if (decoder) {
                const int Cin = 2 * C;
                const RawTensor* w = raw(sidx(P + ".up.", i, ".weight"));
                if (!w || w->numel != (long)Cin * C * 2 * r) return fail("missing/mis-shaped " + sidx(P + ".up.", i, ".weight"));
                GatherSpec g{r, 1, 2L * r, -(long)r, (long)C * 2 * r, C, Cin, Cin};
                if (gather_to_pw(w->d, r * C, 2 * Cin, g, st.resample, nullptr, true)) return 1;
                const float* b = nullptr;
                if (opt_vec(sidx(P + ".up.", i, ".bias"), C, 0.f, &b)) return 1;
                GatherSpec gb{0, 0, 0, 0, 1, 1, C, C};
                PW dummy;
                if (gather_to_pw(b, 1, r * C, gb, dummy, &st.resample_bias)) return 1;
            } else {
                const int Cin = C / 2;
                const RawTensor* w = raw(sidx(P + ".down.", i, ".weight"));
                if (!w || w->numel != (long)C * Cin * 2 * r) return fail("missing/mis-shaped " + sidx(P + ".down.", i, ".weight"));
                GatherSpec g{0, 0, (long)Cin * 2 * r, 1, 2L * r, C, Cin, Cin};
                if (gather_to_pw(w->d, C, 2 * r * Cin, g, st.resample, nullptr)) return 1;
                const float* b = nullptr;
                if (opt_vec(sidx(P + ".down.", i, ".bias"), C, 0.f, &b)) return 1;
                st.resample_bias = const_cast<float*>(b);
            }
        }
        const int depth = decoder ? s.depths[i] : s.depths[S - 1 - i];
        for (int j = 0; j < depth; ++j) {
            std::string p = P + ".stages." + std::to_string(i) + "." + std::to_string(j);
            CodecBlockW b;
            b.norm_w = rawp(p + ".norm.weight");
            b.ffn_norm_w = rawp(p + ".ffn_norm.weight");
            const float* mw = rawp(p + ".mixer.weight");
            {
                const long Fh = (long)s.ffn_mult * C;
                if (check_shape(p + ".norm.weight", {C}) || check_shape(p + ".mixer.weight", {C, Kc}) ||
                    check_shape(p + ".ffn_norm.weight", {C}) || check_shape(p + ".ffn.w1.weight", {Fh, C}) ||
                    check_shape(p + ".ffn.w2.weight", {C, Fh}))
                    return 1;
                if (opt_vec(p + ".mixer.bias", C, 0.f, &b.dw_b) || opt_vec(p + ".gamma", C, 1.f, &b.gamma) ||
                    opt_vec(p + ".ffn.w1.bias", Fh, 0.f, &b.b1) || opt_vec(p + ".ffn.w2.bias", C, 0.f, &b.b2) ||
                    opt_vec(p + ".ffn_gamma", C, 1.f, &b.ffn_gamma))
                    return 1;
            }
            GatherSpec g{0, 0, 1, 0, Kc, Kc, C, C};
            PW dummy;
            if (gather_to_pw(mw, Kc, C, g, dummy, &b.dw_w)) return 1;
            b.w1 = pack_rows({p + ".ffn.w1.weight"});
            b.w2 = pack_rows({p + ".ffn.w2.weight"});
            if (!b.w1.N || !b.w2.N) return fail("codec ffn pack failed: " + p + " " + err_);
            const int F = s.ffn_mult * C;
            if ((C == 128 || C == 256) && F == 4 * C && b.w1.K == C && b.w2.K == F) {  // streamed fused FFN: W2 hidden-tile-major
                b.w2t.hi = static_cast<bf16_t*>(dalloc((size_t)C * F * 2));
                b.w2t.lo = static_cast<bf16_t*>(dalloc((size_t)C * F * 2));
                b.w2t.h16 = static_cast<bf16_t*>(dalloc((size_t)C * F * 2));
                if (!b.w2t.hi || !b.w2t.lo || !b.w2t.h16) return fail("codec w2 tile pack: out of memory");
                HIPC(launch_w2_tile_pack(b.w2.hi, b.w2t.hi, C, F, 0));
                HIPC(launch_w2_tile_pack(b.w2.lo, b.w2t.lo, C, F, 0));
                HIPC(launch_w2_tile_pack(b.w2.h16, b.w2t.h16, C, F, 0));
                b.w2t.N = (F / 32) * C;
                b.w2t.K = 32;
            }
            if (certify_codec_ffn(p, b, C, F)) return 1;
            st.blocks.push_back(b);
        }
        h.stages.push_back(st);
    }
    const int C0 = h.stages[0].C, Cl = h.stages[S - 1].C;
    if (decoder) {
        const RawTensor* w = raw(P + ".stem.weight");
        if (!w || w->numel != (long)C0 * s.latent_dim * Kc) return fail("missing decoder stem");
        GatherSpec g{0, 0, (long)s.latent_dim * Kc, 1, Kc, C0, s.latent_dim, s.latent_dim};
        if (gather_to_pw(w->d, C0, Kc * s.latent_dim, g, h.stem, nullptr)) return 1;
        if (opt_vec(P + ".stem.bias", C0, 0.f, &h.stem_b)) return 1;
        const float* hw = rawp(P + ".head.weight");
        const float* hb = nullptr;
        if (opt_vec(P + ".head.bias", 1, 0.f, &hb)) return 1;
        if (!hw) return fail("missing decoder head");
        if (check_shape(P + ".head.weight", {1, Cl, Kc})) return 1;
        GatherSpec gh{0, 0, 1, 0, Kc, Kc, Cl, Cl};
        PW dummy;
        if (gather_to_pw(hw, Kc, Cl, gh, dummy, &h.head_w)) return 1;
        HIPC(hipMemcpy(&h.head_b_host, hb, 4, hipMemcpyDeviceToHost));
    } else {
        h.stem_w_raw = rawp(P + ".stem.weight");
        const RawTensor* w = raw(P + ".head.weight");
        if (opt_vec(P + ".stem.bias", C0, 0.f, &h.stem_b) || opt_vec(P + ".head.bias", s.latent_dim, 0.f, &h.head_b)) return 1;
        if (!h.stem_w_raw || !w) return fail("missing encoder stem/head");
        if (check_shape(P + ".stem.weight", {C0, 1, Kc}) || check_shape(P + ".head.weight", {s.latent_dim, Cl, Kc})) return 1;
        GatherSpec g{0, 0, (long)Cl * Kc, 1, Kc, s.latent_dim, Cl, Cl};
        if (gather_to_pw(w->d, s.latent_dim, Kc * Cl, g, h.head, nullptr)) return 1;
    }
    // optional RMSNorm in front of the head conv (CodecSpec.final_norm)
    h.final_norm_w = nullptr;
    if (raw(P + ".final_norm.weight")) {
        if (check_shape(P + ".final_norm.weight", {Cl})) return 1;
        h.final_norm_w = rawp(P + ".final_norm.weight");
    }
    h.ready = true;
    return 0;
}

// The fused codec FFN kernels (codec_ffn_wave / codec_ffn_stream: C <= 256) convert their normalised input and their GELU
// hidden to fp16 in registers and are VALU-bound: a per-value range check there would cost every batch ~4 % of the decoder for
// an event the weights can RULE OUT.  The input is RMS-normalised, so both are bounded by the weights alone
// (ffn_range_bound_kernel); a block whose bound stays inside the fp16 range needs no run-time check, one whose bound does not
// is reported through get_saturations (static part of SITE_CODEC_FFN), which makes the host side demote the site.
static constexpr float kFfnCertLimit = 65504.f / 1.002f;
int Engine::certify_codec_ffn(const std::string& name, CodecBlockW& b, int C, int F) {
    if (!(C == 32 || C == 64 || C == 128 || C == 256) || F != 4 * C) return 0;   // the wider stages' hiddens are counted at run time
    if (!cert_scratch_) {   // no scratch: nothing can be certified — the block runs split-bf16, and that is REPORTED
        b.f16_ok = false;
        ++sat_static_[SITE_CODEC_FFN];
        range_report_ += name + ": fused FFN range not certified (no certificate scratch); ";
        return 0;
    }
    const float* w1 = rawp(name + ".ffn.w1.weight");
    if (!w1) return 0;
    HIPC(hipMemsetAsync(cert_scratch_, 0, 2 * sizeof(float), 0));
    HIPC(launch_ffn_range_bound(w1, b.b1, b.ffn_norm_w, F, C, cert_scratch_, 0));
    float bound[2] = {0.f, 0.f};
    HIPC(hipMemcpy(bound, cert_scratch_, sizeof bound, hipMemcpyDeviceToHost));
    const float worst = bound[0] > bound[1] ? bound[0] : bound[1];
    if (worst > range_worst_) range_worst_ = worst;
    // The bound is evaluated on the fp32 weights; the kernels multiply fp16-rounded W1 rows with fp16-rounded inputs (2^-11 relative
    // each), so the hidden they convert can exceed it by ~(1 + 2^-11)^2 = 1.001.  Certified blocks convert WITHOUT a clamp (an
    // inf there turns the packed GELU into NaN), hence a margin instead of the bare fp16 maximum.
    if (!(worst <= kFfnCertLimit)) {
        b.f16_ok = false;
        ++sat_static_[SITE_CODEC_FFN];
        char buf[256];
        snprintf(buf, sizeof buf, "%s: fused FFN hidden bound %.4g, input bound %.4g exceed the fp16 range; ", name.c_str(), bound[0], bound[1]);
        range_report_ += buf;
    }
    return 0;
}
