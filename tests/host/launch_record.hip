// Launch recorder (tests/test_launch_table_cpu.py): the library's launcher objects linked against recording stand-ins for the HIP
// runtime entry points they call (hip_record.hpp).  No GPU is opened.  Every launcher call of the sweep below prints one line: the call, then the
// kernel instantiation, grid, workgroup and dynamic LDS it launched (or the error it returned), and for gemm3_kernel / gemm_kernel the
// host-set switches of the operand struct.  tests/golden/launch_table.txt.gz holds the lines recorded at the last commit that passed
// tuning through globals (its id is the table's first line): which kernel runs for which shape and tuning is pinned line by line.
#include "hip_record.hpp"
#include "kernels.hpp"
#include "prof.hpp"

thread_local Profiler* g_prof = nullptr;   // (engine.hip's, which is not linked)
thread_local const char* g_prof_tag = nullptr;
thread_local int g_prof_shapes = 0;

static int g_launches = 0;   // of the current call
static void on_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, hipStream_t, void** args) {
    printf(" -> ");
    print_launch(name, grid, block, lds, args);
    ++g_launches;
}

// one line per call: "<call> -> <launch>" or "<call> -> err=<hipError_t>" (a call that does neither printed nothing after "->")
template <class F>
static void call(const LaunchTuning& tu, const char* what, F&& f) {
    printf("%s d%d cap%d/%d t%d w%d s%d g%d n%d x%d", what, tu.deep, tu.persist_cus, tu.persist_mask, tu.t160, tu.w4_minm, tu.stage16, tu.group,
           tu.nfast, tu.xcd);
    g_launches = 0;
    const hipError_t e = f();
    if (e != hipSuccess) printf(" -> err=%d", (int)e);
    else if (!g_launches) printf(" -> nothing");
    printf("\n");
}

static const int kM[] = {1, 64, 75, 120, 240, 480, 481, 600, 640, 641, 1024, 1800, 2048, 4800, 24000};
static const int kN[] = {32, 64, 128, 512, 960, 1024, 2048, 3840, 4096, 4864, 8192};
static const int kFmt[] = {PREC_BF16, PREC_F16, PREC_BF16X3};
static float g_dummy;   // a non-null address for the operands whose presence selects a path (never read)

static Gemm3Operands ops3(int M, int N, int K) {
    Gemm3Operands g{};
    g.amap = rowmap_plain(K);
    g.ldw = K; g.M = M; g.N = N; g.K = K;
    g.Wlo = reinterpret_cast<const bf16_t*>(&g_dummy);   // (gemm3_store_x2 requires the lo array)
    return g;
}
static GemmOperands ops(int M, int N, int K) {
    GemmOperands g{};
    g.amap = rowmap_plain(K);
    g.ldw = K; g.M = M; g.N = N; g.K = K; g.xcd_order = 1;
    return g;
}

// every gemm3 entry on one product
static void gemm3_entries(const LaunchTuning& tu, int M, int N, int K, int f, int cfg, bool store_only = false) {
    char w[96];
    const Gemm3Operands g = ops3(M, N, K);
    auto tag = [&](const char* entry) { snprintf(w, sizeof w, "%s f%d %dx%dx%d cfg%d", entry, f, M, N, K, cfg); return w; };
    call(tu, tag("gemm3_store"), [&] { return gemm3_store(g, ACT_NONE, EpiStore<ACT_NONE>{}, 1, f, 0, tu, cfg); });
    if (store_only) return;
    call(tu, tag("gemm3_store_gelu"), [&] { return gemm3_store(g, ACT_GELU, EpiStore<ACT_NONE>{}, 1, f, 0, tu, cfg); });
    if (f == PREC_F16) call(tu, tag("gemm3_store_x2"), [&] { return gemm3_store_x2(g, EpiStore<ACT_NONE>{}, 0, tu, cfg); });
    for (int gate = 0; gate < 3; ++gate) {
        char e[32];
        snprintf(e, sizeof e, "gemm3_resid%d", gate);
        call(tu, tag(e), [&] { return gemm3_resid(g, gate, EpiResid<0>{}, f, 0, tu, cfg); });
    }
    call(tu, tag("gemm3_resid_ln"), [&] { return gemm3_resid_ln(g, EpiResidLN{}, f, 0, tu, cfg); });
    if (cfg >= 0) return;   // the entries below choose their own tile
    call(tu, tag("gemm3_swiglu"), [&] { return gemm3_swiglu(g, EpiSwiGLU{}, f, 0, tu); });
    call(tu, tag("gemm3_kv"), [&] { return gemm3_kv(g, EpiKV{}, f, 0, tu); });
    call(tu, tag("gemm3_convpos"), [&] { return gemm3_convpos(g, false, EpiConvPos<0>{}, 3, f, 0, tu); });
    call(tu, tag("gemm3_convpos_final"), [&] { return gemm3_convpos(g, true, EpiConvPos<0>{}, 3, f, 0, tu); });
    EpiQKV q{};
    q.HW = 64; q.H = N / 256; q.dh = 64; q.prec = f;   // (N that is no whole number of 4 x 64-wide heads: rejected, and recorded as that)
    call(tu, tag("gemm3_qkv"), [&] { return gemm3_qkv(g, q, f, 0, tu); });
    q.fold.part = &g_dummy; q.fold.NP = K / 32;
    call(tu, tag("gemm3_qkv_fold"), [&] { return gemm3_qkv(g, q, f, 0, tu); });
}

static void gemm_entries(const LaunchTuning& tu, int M, int N, int K, int f, bool store_only = false) {
    char w[96];
    const GemmOperands g = ops(M, N, K);
    auto tag = [&](const char* entry) { snprintf(w, sizeof w, "%s f%d %dx%dx%d", entry, f, M, N, K); return w; };
    call(tu, tag("gemm_store"), [&] { return gemm_store(g, ACT_NONE, EpiStore<ACT_NONE>{}, 1, f, 0, tu); });
    if (store_only) return;
    call(tu, tag("gemm_resid"), [&] { return gemm_resid(g, 1, EpiResid<0>{}, f, 0, tu); });
#ifdef SMTTS_TEST_KERNELS
    call(tu, tag("gemm_swiglu"), [&] { return gemm_swiglu(g, EpiSwiGLU{}, f, 0, tu); });
    call(tu, tag("gemm_kv"), [&] { return gemm_kv(g, EpiKV{}, f, 0, tu); });
    call(tu, tag("gemm_convpos"), [&] { return gemm_convpos(g, false, EpiConvPos<0>{}, 3, f, 0, tu); });
#endif
}

static void codec_entries(const LaunchTuning& tu, int M) {
    char w[96];
    auto tag = [&](const char* entry, int C, int f) { snprintf(w, sizeof w, "%s f%d C%d M%d", entry, f, C, M); return w; };
    for (int f : kFmt) {
        for (int C : {128, 256})
            call(tu, tag("ffn_stream", C, f), [&] { return launch_codec_ffn_stream(nullptr, rowmap_plain(C), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, M, C, 4 * C, 1e-6f, f, 0, tu); });
        for (int C : {32, 64}) {
            const RowMap img = rowmap_batched(C, 32, 38L * C, 0);   // utterances of 32 frames + 6 pad frames
            call(tu, tag("ffn_wave", C, f), [&] { return launch_codec_ffn_wave(nullptr, img, nullptr, nullptr, nullptr, C, nullptr, nullptr, nullptr, nullptr, nullptr, M, C, 4 * C, 1e-6f, f, 0, tu); });
            call(tu, tag("block_wave", C, f), [&] {   // (C = 64 at split-bf16: rejected)
                return launch_codec_block_wave(&g_dummy, nullptr, img, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, C, nullptr, nullptr, nullptr, nullptr, nullptr, M, C, 4 * C, 7, 1e-6f, f, 0, tu);
            });
            for (int nb = 1; nb <= 3 && C == 32; ++nb) {   // (split-bf16: rejected)
                const CodecChainBlock blocks[3] = {};
                snprintf(w, sizeof w, "chain_wave%d f%d C%d M%d", nb, f, C, M);
                call(tu, w, [&] { return launch_codec_chain_wave(&g_dummy, nullptr, img, blocks, nb, M, C, 4 * C, 7, 1e-6f, f, 0, tu); });
            }
        }
        for (int K : {256, 128})
            call(tu, tag("upsample_wave", K, f), [&] { return launch_codec_upsample_wave(nullptr, rowmap_plain(K), nullptr, nullptr, K, nullptr, nullptr, rowmap_plain(K / 2), M, K, K / 2, f, 0, tu); });
    }
}

int main() {
    // gemm3: ring depth 1 over three K, depths 0 and 2 at K = 960, the launcher's own tile choice
    for (int deep : {1, 0, 2})
        for (int K : {64, 960, 8192}) {
            if (deep != 1 && K != 960) continue;
            LaunchTuning tu;
            tu.deep = deep;
            for (int f : kFmt)
                for (int M : kM)
                    for (int N : kN) gemm3_entries(tu, M, N, K, f, -1);
        }
    // ... and every explicit tile shape
    for (int cfg = 0; cfg <= 9; ++cfg)
        for (int f : kFmt)
            for (int M : {600, 4800})
                for (int N : {960, 4096}) gemm3_entries(LaunchTuning{}, M, N, 960, f, cfg);
    // the fp32-A kernels
    for (int K : {32, 64, 960})
        for (int f : kFmt)
            for (int M : kM)
                for (int N : kN) gemm_entries(LaunchTuning{}, M, N, K, f);
    // each remaining switch alone at its other value, on the store entries
    for (int sw = 0; sw < 6; ++sw) {
        LaunchTuning tu;
        if (sw == 0) tu.t160 = 0;
        if (sw == 1) tu.nfast = 0;
        if (sw == 2) tu.group = 1;
        if (sw == 3) tu.stage16 = 0;
        if (sw == 4) tu.w4_minm = 2048;
        if (sw == 5) tu.xcd = 0;
        for (int f : kFmt)
            for (int M : {600, 1800, 4800, 24000})
                for (int N : {960, 2048, 4096}) {
                    gemm3_entries(tu, M, N, 960, f, -1, true);
                    gemm_entries(tu, M, N, 960, f, true);
                }
    }
    // the persistent codec kernels under every grid cap and mask
    for (int cap : {0, 192, 300})
        for (int mask : {7, 6, 5, 3}) {
            LaunchTuning tu;
            tu.persist_cus = cap;
            tu.persist_mask = mask;
            for (int M : {32, 1024, 4800, 24000, 192000}) codec_entries(tu, M);
        }
    return 0;
}
