// Engine, the latent scorers: the recogniser (asr.hip) and the speaker verifier (sv.hip), finalize and entry points.
#include "engine_impl.hpp"
#include "scorer_pack.hpp"

// a tensor of the registry to the host, a packed vector to the device (an allocation of this finalize), the BatchNorm fold of the
// four tensors behind a prefix
struct Engine::ScorerPack {
    Engine& e;
    bool bad = false;      // a copy or an allocation failed
    bool bn_bad = false;   // a running_var was refused: the engine's error names the first
    std::vector<float> host(const std::string& n) {
        const RawTensor* t = e.raw(n);
        std::vector<float> v((size_t)t->numel);
        if (hipMemcpy(v.data(), t->d, v.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) bad = true;
        return v;
    }
    const float* up(const std::vector<float>& v) {
        float* d = static_cast<float*>(e.dalloc(v.size() * 4));
        if (!d || hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { bad = true; return nullptr; }
        return d;
    }
    const float* blocks(const std::string& n, long n_out, long i_all, long i_use, long taps, long n_pad) {
        return up(pack_blocks64(host(n), n_out, i_all, i_use, taps, n_pad));
    }
    const float* cols(const std::string& n, long n_out, long i_all, long i0, long i_use) { return up(pack_cols(host(n), n_out, i_all, i0, i_use)); }
    void fold(const std::string& p, const float*& scale, const float*& shift) {   // p + weight / bias / running_mean / running_var
        std::vector<float> sc, sh;
        if (!fold_batchnorm(host(p + "weight"), host(p + "bias"), host(p + "running_mean"), host(p + "running_var"), sc, sh)) {
            if (!bn_bad) e.fail("tensor " + p + "running_var has a negative (or NaN) entry");
            bn_bad = true;
            return;
        }
        scale = up(sc); shift = up(sh);
    }
};

int Engine::scorer_entry(const char* entry, const char* net, const char* part, const char* out, bool ready, int n_min,
                         size_t (*ws_need)(int, int), const float* x, const int32_t* n_len, int B, int N, const void* ws, size_t ws_bytes,
                         const float* result) {
    const std::string E = std::string("smtts_") + entry + ": ";
    if (!ready) return fail(E + "this engine holds no " + part + " (load the " + net + ".* tensors and finalize)");
    if (B < 1 || B > 64 || N < n_min || N > 225) return fail(E + "B must be in [1, 64] and N in [" + std::to_string(n_min) + ", 225]");
    if (!x || !n_len || !ws || !result) return fail(E + "a required pointer is NULL");
    if ((uintptr_t)ws & 255) return fail(E + "the workspace must be 256-byte aligned");
    if (ws_bytes < ws_need(B, N)) return fail(E + "workspace too small (smtts_" + net + "_workspace_bytes)");
    if (((uintptr_t)x | (uintptr_t)n_len | (uintptr_t)result) & 3) return fail(E + "x, n_len and " + out + " must be 4-byte aligned");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// recogniser (asr.hip): shapes by name, then the packs its kernels read
// ---------------------------------------------------------------------------------------------
int Engine::finalize_asr() {
    constexpr long D = 64, FF = 1024, C = 198, L = 7, KC = 9;
    const std::string EL = "asr.encoder.conformer_layers.";
    if (check_shape("asr.upsample.deconv.weight", {D, 1, 4}) || check_shape("asr.upsample.deconv.bias", {D}) ||
        check_shape("asr.proj.weight", {C, D}) || check_shape("asr.proj.bias", {C}))
        return 1;
    for (int l = 0; l < L; ++l) {
        const std::string p = EL + std::to_string(l) + ".";
        for (const char* f : {"ffn1", "ffn2"}) {
            const std::string q = p + f + ".sequential.";
            if (check_shape(q + "0.weight", {D}) || check_shape(q + "0.bias", {D}) || check_shape(q + "1.weight", {FF, D}) ||
                check_shape(q + "1.bias", {FF}) || check_shape(q + "4.weight", {D, FF}) || check_shape(q + "4.bias", {D}))
                return 1;
        }
        for (const char* n : {"self_attn_layer_norm", "conv_module.layer_norm", "final_layer_norm", "conv_module.sequential.3"})
            if (check_shape(p + n + ".weight", {D}) || check_shape(p + n + ".bias", {D})) return 1;
        const std::string c = p + "conv_module.sequential.";
        if (check_shape(p + "self_attn.in_proj_weight", {3 * D, D}) || check_shape(p + "self_attn.in_proj_bias", {3 * D}) ||
            check_shape(p + "self_attn.out_proj.weight", {D, D}) || check_shape(p + "self_attn.out_proj.bias", {D}) ||
            check_shape(c + "0.weight", {2 * D, D, 1}) || check_shape(c + "0.bias", {2 * D}) || check_shape(c + "2.weight", {D, 1, KC}) ||
            check_shape(c + "2.bias", {D}) || check_shape(c + "3.running_mean", {D}) || check_shape(c + "3.running_var", {D}) ||
            check_shape(c + "5.weight", {D, D, 1}) || check_shape(c + "5.bias", {D}))
            return 1;
    }
    ScorerPack pk{*this};
    // W (n_out, k_in) row-major -> blocks of 64 outputs x 64 inputs, each [k][n] (scorer_pack.hpp; n_pad: zero columns behind n_out)
    auto blocks_t = [&](const std::string& n, long n_out, long k_in, long n_pad) { return pk.blocks(n, n_out, k_in, k_in, 1, n_pad); };
    asr_.up_w = rawp("asr.upsample.deconv.weight");
    asr_.up_b = rawp("asr.upsample.deconv.bias");
    for (int l = 0; l < L; ++l) {
        const std::string p = EL + std::to_string(l) + ".";
        AsrLayerW& w = asr_.layer[l];
        for (int f = 0; f < 2; ++f) {
            const std::string q = p + (f ? "ffn2" : "ffn1") + ".sequential.";
            AsrFfnW& g = f ? w.ffn2 : w.ffn1;
            g.ln_w = rawp(q + "0.weight"); g.ln_b = rawp(q + "0.bias");
            g.w1t = blocks_t(q + "1.weight", FF, D, FF); g.b1 = rawp(q + "1.bias");
            g.w2t = blocks_t(q + "4.weight", D, FF, D); g.b2 = rawp(q + "4.bias");
        }
        w.aln_w = rawp(p + "self_attn_layer_norm.weight"); w.aln_b = rawp(p + "self_attn_layer_norm.bias");
        w.wqkv_t = blocks_t(p + "self_attn.in_proj_weight", 3 * D, D, 3 * D); w.bqkv = rawp(p + "self_attn.in_proj_bias");
        w.wo_t = blocks_t(p + "self_attn.out_proj.weight", D, D, D); w.bo = rawp(p + "self_attn.out_proj.bias");
        const std::string c = p + "conv_module.sequential.";
        w.conv.ln_w = rawp(p + "conv_module.layer_norm.weight"); w.conv.ln_b = rawp(p + "conv_module.layer_norm.bias");
        w.conv.pw1t = blocks_t(c + "0.weight", 2 * D, D, 2 * D); w.conv.pw1b = rawp(c + "0.bias");
        w.conv.dw_w = rawp(c + "2.weight"); w.conv.dw_b = rawp(c + "2.bias");
        pk.fold(c + "3.", w.conv.bn_scale, w.conv.bn_shift);
        if (pk.bn_bad) return 1;
        w.conv.pw2t = blocks_t(c + "5.weight", D, D, D); w.conv.pw2b = rawp(c + "5.bias");
        w.fln_w = rawp(p + "final_layer_norm.weight"); w.fln_b = rawp(p + "final_layer_norm.bias");
    }
    asr_.proj_t = blocks_t("asr.proj.weight", C, D, 256);
    {
        std::vector<float> pb = pk.host("asr.proj.bias");
        pb.resize(256, 0.f);
        asr_.proj_b = pk.up(pb);
    }
    if (pk.bad) return fail("finalize: packing the recogniser weights failed (device memory)");
    asr_ready_ = true;
    return 0;
}

size_t Engine::asr_workspace_bytes(int B, int N) {
    if (B < 1 || B > 64 || N < 1 || N > 225) { fail("smtts_asr_workspace_bytes: B must be in [1, 64] and N in [1, 225]"); return 0; }
    return asr_ws_bytes(B, N);
}

int Engine::asr_logprobs(hipStream_t st, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes, float* logp) {
    if (scorer_entry("asr_logprobs", "asr", "recogniser", "logp", asr_ready_, 1, asr_ws_bytes, x, n_len, B, N, ws, ws_bytes, logp)) return 1;
    HIPC(hipSetDevice(device_));
    ProfTag tag("asr");
    const hipError_t e = launch_asr_logprobs(asr_, x, n_len, B, N, ws, logp, st);
    return e == hipSuccess ? 0 : fail_hip(e, "asr_logprobs");
}

// ---------------------------------------------------------------------------------------------
// speaker verifier (sv.hip): shapes by name, then the packs its kernels read
// ---------------------------------------------------------------------------------------------
int Engine::finalize_sv() {
    constexpr long C = 768, BAND = 64, SE = 192, ATT = 192, MFA = 2304, POOL = 4608, EMB = 192, IN = 64;
    static const int DIL[3] = {2, 3, 5};
    const std::string EC = "sv.ecapa.";
    auto chk_conv = [&](const std::string& p, long o, long i, long k) {
        return check_shape(p + ".conv.weight", {o, i, k}) || check_shape(p + ".conv.bias", {o});
    };
    auto chk_norm = [&](const std::string& p, long n) {
        for (const char* leaf : {"weight", "bias", "running_mean", "running_var"})
            if (check_shape(p + ".norm." + leaf, {n})) return 1;
        return 0;
    };
    auto chk_tdnn = [&](const std::string& p, long i, long o, long k) { return chk_conv(p + ".conv", o, i, k) || chk_norm(p + ".norm", o); };
    if (chk_tdnn(EC + "blocks.0", IN, C, 3) || chk_tdnn(EC + "mfa", MFA, MFA, 1) || chk_tdnn(EC + "asp.tdnn", 3 * MFA, ATT, 1) ||
        chk_conv(EC + "asp.conv", MFA, ATT, 1) || chk_norm(EC + "asp_bn", POOL) || chk_conv(EC + "fc", EMB, POOL, 1))
        return 1;
    for (int i = 1; i <= 3; ++i) {
        const std::string p = EC + "blocks." + std::to_string(i) + ".";
        if (chk_tdnn(p + "tdnn1", C, C, 1) || chk_tdnn(p + "tdnn2", C, C, 1) || chk_conv(p + "se_block.conv1", SE, C, 1) ||
            chk_conv(p + "se_block.conv2", C, SE, 1))
            return 1;
        for (int j = 0; j < 11; ++j)
            if (chk_tdnn(p + "res2net_block.blocks." + std::to_string(j), BAND, BAND, 3)) return 1;
    }
    ScorerPack pk{*this};
    // conv weight (n_out, i_all, taps), input channels [0, i_use) -> 64 x 64 blocks [k][n], k = tap * i_use + channel (scorer_pack.hpp)
    auto blocks_t = [&](const std::string& n, long n_out, long i_all, long i_use, long taps) { return pk.blocks(n, n_out, i_all, i_use, taps, n_out); };
    auto cols_t = [&](const std::string& n, long n_out, long i_all, long i0, long i_use) { return pk.cols(n, n_out, i_all, i0, i_use); };
    auto tdnn = [&](const std::string& p, long i, long i_use, long o, long k) {
        SvTdnnW t{};
        t.wt = blocks_t(p + ".conv.conv.weight", o, i, i_use, k);
        t.b = rawp(p + ".conv.conv.bias");
        pk.fold(p + ".norm.norm.", t.scale, t.shift);
        return t;
    };
    sv_.in = tdnn(EC + "blocks.0", IN, IN, C, 3);
    for (int i = 0; i < 3; ++i) {
        const std::string p = EC + "blocks." + std::to_string(i + 1) + ".";
        SvBlockW& b = sv_.block[i];
        b.tdnn1 = tdnn(p + "tdnn1", C, C, C, 1);
        for (int j = 0; j < 11; ++j) b.band[j] = tdnn(p + "res2net_block.blocks." + std::to_string(j), BAND, BAND, BAND, 3);
        b.tdnn2 = tdnn(p + "tdnn2", C, C, C, 1);
        b.se_w1t = cols_t(p + "se_block.conv1.conv.weight", SE, C, 0, C); b.se_b1 = rawp(p + "se_block.conv1.conv.bias");
        b.se_w2t = cols_t(p + "se_block.conv2.conv.weight", C, SE, 0, SE); b.se_b2 = rawp(p + "se_block.conv2.conv.bias");
        b.dil = DIL[i];
    }
    sv_.mfa = tdnn(EC + "mfa", MFA, MFA, MFA, 1);
    sv_.att = tdnn(EC + "asp.tdnn", 3 * MFA, MFA, ATT, 1);
    sv_.att_ct = cols_t(EC + "asp.tdnn.conv.conv.weight", ATT, 3 * MFA, MFA, POOL);
    sv_.logit = SvTdnnW{blocks_t(EC + "asp.conv.conv.weight", MFA, ATT, ATT, 1), rawp(EC + "asp.conv.conv.bias"), nullptr, nullptr};
    pk.fold(EC + "asp_bn.norm.", sv_.pool_scale, sv_.pool_shift);
    sv_.fc_t = cols_t(EC + "fc.conv.weight", EMB, POOL, 0, POOL);
    sv_.fc_b = rawp(EC + "fc.conv.bias");
    if (pk.bn_bad) return 1;
    if (pk.bad) return fail("finalize: packing the verifier weights failed (device memory)");
    sv_ready_ = true;
    return 0;
}

size_t Engine::sv_workspace_bytes(int B, int N) {
    if (B < 1 || B > 64 || N < 6 || N > 225) { fail("smtts_sv_workspace_bytes: B must be in [1, 64] and N in [6, 225]"); return 0; }
    return sv_ws_bytes(B, N);
}

int Engine::sv_embed(hipStream_t st, const float* x, const int32_t* n_len, int B, int N, void* ws, size_t ws_bytes, float* emb) {
    if (scorer_entry("sv_embed", "sv", "speaker verifier", "emb", sv_ready_, 6, sv_ws_bytes, x, n_len, B, N, ws, ws_bytes, emb)) return 1;
    HIPC(hipSetDevice(device_));
    ProfTag tag("sv");
    const hipError_t e = launch_sv_embed(sv_, x, n_len, B, N, ws, emb, st);
    return e == hipSuccess ? 0 : fail_hip(e, "sv_embed");
}
