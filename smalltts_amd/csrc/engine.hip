// Engine: construction, tuning and profiling, the tensor registry, the GEMM packing helpers and the finalize() dispatcher.  The parts
// it dispatches to and the operators live in the engine_*.hip units (engine_impl.hpp: what they share).
#include "engine_impl.hpp"

thread_local Profiler* g_prof = nullptr;
thread_local const char* g_prof_tag = nullptr;
thread_local int g_prof_shapes = 0;

Engine::Engine(int device) : device_(device) {
    set_precision(kDefaultPrecision);
    if (const char* nf = lab_env("SMTTS_GEMM_NFAST")) tune_.nfast = atoi(nf);
    if (const char* gg = getenv("SMTTS_GEMM_GROUP")) tune_.group = atoi(gg);
    if (const char* gx = getenv("SMTTS_GEMM_XCD")) tune_.xcd = atoi(gx);
    if (const char* pc = getenv("SMTTS_PERSIST_CUS")) persist_cus_tp_ = atoi(pc);
    if (const char* pm = lab_env("SMTTS_PERSIST_MASK")) tune_.persist_mask = atoi(pm);
    if (const char* dp = getenv("SMTTS_GEMM_DEEP")) tune_.deep = atoi(dp);
    if (const char* s16 = lab_env("SMTTS_GEMM_STAGE16")) tune_.stage16 = atoi(s16);
    if (const char* w4 = lab_env("SMTTS_GEMM_W4_MINM")) tune_.w4_minm = atoi(w4);
    if (const char* t1 = lab_env("SMTTS_GEMM_T160")) tune_.t160 = atoi(t1);
    const char* s = getenv("SMTTS_SINGLE_STREAM");
    if (s && *s == '1') dual_stream_ = false;
    if ((s = lab_env("SMTTS_BLOCK_WAVE"))) block_wave_ = atoi(s) != 0;
    if ((s = getenv("SMTTS_STAGE_CHAIN"))) { stage_chain_ = atoi(s) != 0; if (atoi(s) >= 2) chain_min_run_ = 0; }   // 2: the chain whatever the run length (tests)
    if ((s = lab_env("SMTTS_CHAIN_MIN"))) chain_min_blocks_ = atoi(s);
    if ((s = lab_env("SMTTS_CHAIN_MIN_RUN"))) chain_min_run_ = atoi(s);
    if ((s = lab_env("SMTTS_SMALLM_SPLITK"))) small_m_splitk_ = atoi(s) != 0;
    if ((s = lab_env("SMTTS_CONVPOS_BY_GROUP"))) convpos_by_group_ = atoi(s) != 0;
    if ((s = getenv("SMTTS_ATTN_EPI"))) attn_epi_ = atoi(s) != 0;
    if ((s = lab_env("SMTTS_ATTN_IMG"))) attn_img_ = atoi(s) != 0;
    if ((s = getenv("SMTTS_LN_FOLD"))) ln_fold_ = atoi(s) != 0;
    if ((s = lab_env("SMTTS_LN_FOLD_TP"))) ln_fold_tp_ = atoi(s) != 0;
    if ((s = lab_env("SMTTS_UP_G3_MINK")) && atoi(s) >= 64) up_g3_mink_ = atoi(s);
    if ((s = getenv("SMTTS_MIXER_WIDE"))) mixer_wide_ = atoi(s) != 0;
    if ((s = lab_env("SMTTS_X2_MINK")) && atoi(s) >= 64) x2_mink_ = atoi(s);
    if ((s = lab_env("SMTTS_X2_MAXK")) && atoi(s) >= 64) x2_maxk_ = atoi(s);
    if ((s = lab_env("SMTTS_KSPLIT_OUT")) && atoi(s) >= 1 && atoi(s) <= kSplitK) ksplit_out_ = atoi(s);
    if ((s = lab_env("SMTTS_KSPLIT_ENC")) && atoi(s) >= 1 && atoi(s) <= kSplitK) ksplit_enc_ = atoi(s);
    if ((s = lab_env("SMTTS_KSPLIT_FF2")) && atoi(s) >= 1 && atoi(s) <= kSplitK) ksplit_ff2_ = atoi(s);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) num_cus_ = cus;
    // three quarters of the CUs, in whole rounds of the 32 shader engines the dispatcher deals workgroups to (measured in flight,
    // ms per batch at 256 / 224 / 208 / 192 / 176 / 160 / 128 workgroups: 8.62 / 8.46 / 8.55 / 8.41 / 8.49 / 8.44 / 8.54)
    if (!getenv("SMTTS_PERSIST_CUS")) persist_cus_tp_ = num_cus_ >= 64 ? num_cus_ * 3 / 4 / 32 * 32 : 0;
    // fp16 range guard: one saturation counter per precision site (+ two floats of scratch for finalize's certificates)
    if (hipSetDevice(device) == hipSuccess) {
        sat_ = static_cast<unsigned*>(dalloc((SITE_COUNT + 2) * sizeof(unsigned)));
        if (sat_ && hipMemset(sat_, 0, (SITE_COUNT + 2) * sizeof(unsigned)) != hipSuccess) sat_ = nullptr;
        if (sat_) cert_scratch_ = reinterpret_cast<float*>(sat_ + SITE_COUNT);
    }
}

int Engine::get_saturations(unsigned* out, int n, bool reset) {
    HIPC(hipSetDevice(device_));
    HIPC(hipDeviceSynchronize());
    unsigned dev[SITE_COUNT] = {};
    if (sat_) HIPC(hipMemcpy(dev, sat_, sizeof dev, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) out[i] = i < SITE_COUNT ? dev[i] + sat_static_[i] : 0u;
    if (reset && sat_) HIPC(hipMemset(sat_, 0, sizeof dev));   // (the static part is a property of the weights: it stays)
    return 0;
}

int Engine::peek_saturations(unsigned* out, int n) {
    HIPC(hipSetDevice(device_));
    unsigned dev[SITE_COUNT] = {};
    if (sat_) HIPC(hipMemcpy(dev, sat_, sizeof dev, hipMemcpyDeviceToHost));   // no device-wide wait, no reset: work in flight goes on counting
    for (int i = 0; i < n; ++i) out[i] = i < SITE_COUNT ? dev[i] + sat_static_[i] : 0u;
    return 0;
}

void Engine::set_tuning(int mode) {
    if (mode == TUNE_THROUGHPUT) {
        if (tuning_ != TUNE_THROUGHPUT) dual_stream_latency_ = dual_stream_;
        tuning_ = TUNE_THROUGHPUT;
        // (A/B only: side streams with batches in flight.  Round 6 gave every caller stream its OWN side stream — three batches in flight
        // then drive six streams, and the batch goes from 7.96 to 9.59 ms (profiles/r06j_ab_dual_tp.txt): more streams than hardware
        // queues serialise worse than one text encoder behind its style encoder.  Stays off.)
        dual_stream_ = lab_env("SMTTS_DUAL_TP") && atoi(lab_env("SMTTS_DUAL_TP")) != 0;
        // Ring depth with batches in flight: round 2 measured shallow rings ahead (10.14 vs 10.38 ms: a workgroup holding 64-128 KiB
        // of LDS while it waits kept the other streams' kernels off its CU).  Re-measured at the end of round 3 — fp16 operand images,
        // shorter epilogues, persistent codec grids capped — deep rings win: 8.53 -> 8.42 ms (profiles/r03ag_*).
        tune_.deep = getenv("SMTTS_GEMM_DEEP") ? atoi(getenv("SMTTS_GEMM_DEEP")) : 1;
        tune_.persist_cus = persist_cus_tp_;
    } else {
        if (tuning_ == TUNE_THROUGHPUT) dual_stream_ = dual_stream_latency_;
        tuning_ = TUNE_LATENCY;
        tune_.persist_cus = 0;
        tune_.deep = getenv("SMTTS_GEMM_DEEP") ? atoi(getenv("SMTTS_GEMM_DEEP")) : 1;
    }
}

void Engine::profile_enable(int mode) {
    const bool on = mode != 0;
    prof_on_ = on;
    prof_.reset();
    g_prof = on ? &prof_ : nullptr;
    g_prof_tag = mode >= 2 ? "" : nullptr;  // 2 = tagged: kernel names carry the pipeline phase
    g_prof_shapes = mode == 3;               // 3 = tagged + the GEMM classes carry their product's shape
}

std::string Engine::profile_report() {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    auto agg = prof_.collect();
    std::string out = "[";
    bool first = true;
    char buf[512];
    for (auto& kv : agg) {
        snprintf(buf, sizeof buf, "%s{\"name\": \"%s\", \"launches\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e, \"bytes8d\": %.6e}",
                 first ? "" : ", ", kv.first.c_str(), kv.second.launches, kv.second.ms, kv.second.flops, kv.second.bytes, kv.second.bytes8d);
        out += buf;
        first = false;
    }
    prof_.reset();
    return out + "]";
}

Engine::~Engine() {
    if (g_prof == &prof_) g_prof = nullptr;
    (void)hipSetDevice(device_);
    for (auto& kv : aux_sets_) {
        (void)hipStreamDestroy(kv.second.stream);
        (void)hipEventDestroy(kv.second.fork);
        (void)hipEventDestroy(kv.second.join);
    }
    for (void* p : allocs_) (void)hipFree(p);
    for (void* p : pack_allocs_) (void)hipFree(p);
}

int Engine::fail_hip(hipError_t e, const char* what) {
    err_ = std::string(what) + ": " + hipGetErrorString(e);
    return 1;
}

void* Engine::dalloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    (packing_ ? pack_allocs_ : allocs_).push_back(p);
    return p;
}

void Engine::free_packs() {
    for (void* p : pack_allocs_) (void)hipFree(p);
    pack_allocs_.clear();
}

int Engine::check_shape(const std::string& name, std::initializer_list<long> want) {
    const RawTensor* t = raw(name);
    if (!t) return fail("missing tensor " + name);
    if (t->shape.size() == want.size() && std::equal(want.begin(), want.end(), t->shape.begin())) return 0;
    auto str = [](auto b, auto e) { std::string o = "("; for (auto i = b; i != e; ++i) o += (i == b ? "" : ", ") + std::to_string(*i); return o + ")"; };
    return fail("tensor " + name + " has shape " + str(t->shape.begin(), t->shape.end()) + ", this build expects " +
                str(want.begin(), want.end()));
}

const RawTensor* Engine::raw(const std::string& n) const {
    auto it = raw_.find(n);
    return it == raw_.end() ? nullptr : &it->second;
}
const float* Engine::rawp(const std::string& n) const {
    const RawTensor* t = raw(n);
    return t ? t->d : nullptr;
}

// ---------------------------------------------------------------------------------------------
// weights in
// ---------------------------------------------------------------------------------------------
int Engine::set_tensor(const char* name, const float* data, const long* shape, int ndim, bool src_on_device) {
    HIPC(hipSetDevice(device_));
    RawTensor t;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
    auto it = raw_.find(name);
    if (it != raw_.end() && it->second.numel == t.numel) {
        t.d = it->second.d;
    } else {
        t.d = static_cast<float*>(dalloc(t.numel * sizeof(float)));
        if (!t.d) return fail("out of device memory for tensor " + std::string(name));
    }
    HIPC(hipMemcpy(t.d, data, t.numel * sizeof(float), src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    raw_[name] = t;
    invalidate();
    return 0;
}

int Engine::synth_tensor(const char* name, const long* shape, int ndim, uint64_t key, float mean, float half_range) {
    HIPC(hipSetDevice(device_));
    RawTensor t;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); t.numel *= shape[i]; }
    t.d = static_cast<float*>(dalloc(t.numel * sizeof(float)));
    if (!t.d) return fail("out of device memory for tensor " + std::string(name));
    HIPC(launch_synth(t.d, t.numel, key, mean, half_range, 0));
    raw_[name] = t;
    invalidate();
    return 0;
}

int Engine::get_tensor(const char* name, float* host_out, long numel) {
    const RawTensor* t = raw(name);
    if (!t) return fail("unknown tensor " + std::string(name));
    if (numel != t->numel) return fail("size mismatch reading tensor " + std::string(name));
    HIPC(hipSetDevice(device_));
    HIPC(hipMemcpy(host_out, t->d, numel * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int Engine::set_codec_spec(const CodecSpecC& s) {
    if (s.n_ratios < 1 || s.n_ratios > 7) return fail("codec spec: 1..7 ratios supported");
    cspec_ = s;
    invalidate();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// packing helpers
// ---------------------------------------------------------------------------------------------
PW Engine::pack_from_f32(const float* src, int N, int K, int k_pad, int n_pad) {
    PW w;
    const int Kp = k_pad > K ? k_pad : K;
    const int Np = n_pad > N ? n_pad : N;  // extra all-zero rows (allocation only; w.N stays the logical row count)
    w.N = N;
    w.K = Kp;
    w.hi = static_cast<bf16_t*>(dalloc((size_t)Np * Kp * 2));
    w.lo = static_cast<bf16_t*>(dalloc((size_t)Np * Kp * 2));
    w.h16 = static_cast<bf16_t*>(dalloc((size_t)Np * Kp * 2));
    if (!w.hi || !w.lo || !w.h16) { w.N = 0; return w; }
    if (Kp != K || Np != N) {
        (void)hipMemsetAsync(w.hi, 0, (size_t)Np * Kp * 2, 0);
        (void)hipMemsetAsync(w.lo, 0, (size_t)Np * Kp * 2, 0);
        (void)hipMemsetAsync(w.h16, 0, (size_t)Np * Kp * 2, 0);
    }
    if (launch_split_rows(src, K, w.hi, w.lo, Kp, N, K, nullptr, 0, w.h16) != hipSuccess) w.N = 0;
    return w;
}

PW Engine::pack_rows(const std::vector<std::string>& names, const std::vector<int>* perm, int k_pad) {
    PW w;
    int K = -1, Ntot = 0;
    for (auto& n : names) {
        const RawTensor* t = raw(n);
        if (!t || t->shape.size() != 2) { err_ = "pack: missing/non-2D tensor " + n; return w; }
        if (K < 0) K = (int)t->shape[1];
        if (K != t->shape[1]) { err_ = "pack: K mismatch at " + n; return w; }
        Ntot += (int)t->shape[0];
    }
    if (names.size() == 1 && !perm) return pack_from_f32(raw(names[0])->d, Ntot, K, k_pad);
    float* tmp = nullptr;
    if (hipMalloc(&tmp, (size_t)Ntot * K * 4) != hipSuccess) { err_ = "pack: temp alloc failed"; return w; }
    long off = 0;
    for (auto& n : names) {
        const RawTensor* t = raw(n);
        (void)hipMemcpyAsync(tmp + off, t->d, t->numel * 4, hipMemcpyDeviceToDevice, 0);
        off += t->numel;
    }
    int* dperm = nullptr;
    if (perm) {
        if (hipMalloc(&dperm, perm->size() * sizeof(int)) != hipSuccess) { (void)hipFree(tmp); return w; }
        (void)hipMemcpyAsync(dperm, perm->data(), perm->size() * sizeof(int), hipMemcpyHostToDevice, 0);
    }
    const int Nout = perm ? (int)perm->size() : Ntot;   // a permutation may also insert zero rows (entries -1): head padding
    w.N = Nout;
    w.K = K;
    w.hi = static_cast<bf16_t*>(dalloc((size_t)Nout * K * 2));
    w.lo = static_cast<bf16_t*>(dalloc((size_t)Nout * K * 2));
    w.h16 = static_cast<bf16_t*>(dalloc((size_t)Nout * K * 2));
    if (!w.hi || !w.lo || !w.h16 || launch_split_rows(tmp, K, w.hi, w.lo, K, Nout, K, dperm, 0, w.h16) != hipSuccess) w.N = 0;
    (void)hipStreamSynchronize(0);
    (void)hipFree(tmp);
    if (dperm) (void)hipFree(dperm);
    return w;
}

// concatenate 1-D tensors; a name "" inserts zero_len[k] zeros (k-th empty name)
float* Engine::concat_vec(const std::vector<std::string>& names, const std::vector<int>& zero_len) {
    long tot = 0;
    size_t zi = 0;
    for (auto& n : names) {
        if (n.empty()) { tot += zero_len[zi++]; continue; }
        const RawTensor* t = raw(n);
        if (!t) { err_ = "concat: missing tensor " + n; return nullptr; }
        tot += t->numel;
    }
    float* d = static_cast<float*>(dalloc(tot * 4));
    if (!d) return nullptr;
    (void)hipMemsetAsync(d, 0, tot * 4, 0);
    long off = 0;
    zi = 0;
    for (auto& n : names) {
        if (n.empty()) { off += zero_len[zi++]; continue; }
        const RawTensor* t = raw(n);
        (void)hipMemcpyAsync(d + off, t->d, t->numel * 4, hipMemcpyDeviceToDevice, 0);
        off += t->numel;
    }
    return d;
}

int Engine::finalize() {
    HIPC(hipSetDevice(device_));
    HIPC(hipDeviceSynchronize());  // nothing in flight may still read the packs of an earlier finalize()
    invalidate();
    free_packs();
    for (unsigned& v : sat_static_) v = 0;
    range_report_.clear();
    range_worst_ = 0.f;
    struct PackMode { bool& f; explicit PackMode(bool& b) : f(b) { f = true; } ~PackMode() { f = false; } } pm(packing_);
    if (raw("velocity.weight")) {
        if (finalize_dit()) return 1;
    }
    if (raw("codec.decoder.stem.weight")) {
        if (finalize_codec(true)) return 1;
    }
    if (raw("codec.encoder.stem.weight")) {
        if (finalize_codec(false)) return 1;
    }
    if (raw("asr.proj.weight")) {
        if (finalize_asr()) return 1;
    }
    if (raw("sv.ecapa.fc.conv.weight")) {
        if (finalize_sv()) return 1;
    }
    HIPC(hipDeviceSynchronize());
    finalized_ = true;
    return 0;
}
