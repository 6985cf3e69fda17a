// Enqueue recorder (tests/test_enqueue_table_cpu.py): the WHOLE library — engine and C ABI included — linked against the recording
// stand-ins of hip_record.hpp.  No GPU is opened.  The program drives the C ABI of include/smalltts_hip.h only: it registers the weight
// inventories it is handed (argv[1]: the DiT, argv[2]: a small codec, the recogniser and the verifier; one "name dim dim ..." line per
// tensor) with smtts_synth_tensor, finalizes, and makes the operator calls below under both tunings and the f16 / bf16x3 presets.  Each call prints a header line "== <call>", then one line per
// runtime call the operator made while it was being enqueued — the stream (main, main2: the caller's; side<k>: the engine's, in order of
// creation), then a kernel launch as launch_record prints it, "memset <bytes>", "memcpy <bytes> <kind>", "record ev<k>", "wait ev<k>";
// "create side<k>" / "create ev<k>" stand alone — then "rc=<code>" and, if non-zero, the error string.  No pointers, no workspace
// offsets or sizes.  tests/golden/enqueue_table.txt.gz holds the lines recorded at the commit its first line names: what an engine
// call enqueues, in which order, on which stream, is pinned line by line.
#include <cstdint>
#include <fstream>
#include <sstream>
#include <vector>

#include "../../include/smalltts_hip.h"
#include "hip_record.hpp"

static void on_launch(const std::string& name, dim3 grid, dim3 block, size_t lds, hipStream_t st, void** args) {
    if (!g_rec_on) return;
    printf("%s ", rec_name(st));
    print_launch(name, grid, block, lds, args);
    printf("\n");
}

static smtts_handle H;
template <class F>
static int call(const std::string& what, F&& f) {
    printf("== %s\n", what.c_str());
    g_rec_on = true;
    const int rc = f();
    g_rec_on = false;
    rec_allocs().clear();
    if (rc) printf("rc=%d %s\n", rc, smtts_last_error(H));
    else printf("rc=0\n");
    return rc;
}

// "device" buffers of the caller: never touched, alive until the program ends
static std::vector<void*> g_dev;
template <class T>
static T* dev(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) { fprintf(stderr, "enqueue_record: out of memory\n"); exit(2); }
    g_dev.push_back(p);
    return static_cast<T*>(p);
}

static const int B = 2, R = 3, P = 5, STEPS = 2, NMAX = 9;

struct Bufs {   // sized for 3B rows (cfg) and N = NMAX
    float *ref, *k_ref, *v_ref, *k_text, *v_text, *x, *v, *t, *noise, *steps, *rope, *mass, *x_pin, *mod, *mod_out, *big[5];
    int64_t *ref_len, *ids;
    uint8_t *ph_mask, *ref_mask, *mask, *pin;
    Bufs() {
        const size_t Bd = 3 * B;
        ref = dev<float>(Bd * R * 64); ref_len = dev<int64_t>(Bd); ids = dev<int64_t>(Bd * P);
        ph_mask = dev<uint8_t>(Bd * P); ref_mask = dev<uint8_t>(Bd * R); mask = dev<uint8_t>(Bd * NMAX); pin = dev<uint8_t>(Bd * NMAX);
        k_ref = dev<float>(12 * Bd * 8 * R * 120); v_ref = dev<float>(12 * Bd * 8 * R * 120);
        k_text = dev<float>(12 * Bd * 8 * P * 120); v_text = dev<float>(12 * Bd * 8 * P * 120);
        x = dev<float>(Bd * NMAX * 960); v = dev<float>(Bd * NMAX * 64); t = dev<float>(Bd);
        noise = dev<float>(STEPS * Bd * NMAX * 64); steps = dev<float>(STEPS * Bd * NMAX * 64); rope = dev<float>(NMAX * 64);
        mass = dev<float>(Bd * NMAX * P); x_pin = dev<float>(Bd * NMAX * 64); mod = dev<float>(Bd * 71040); mod_out = dev<float>(Bd * 71040);
        for (float*& b : big) b = dev<float>(12 * Bd * 8 * NMAX * 120);
    }
};

// the codec of the second inventory: n_filters = 8, depth 1 everywhere (decoder channels 512 .. 8: every codec path)
static const int kRatios[6] = {8, 5, 5, 4, 2, 2}, kDepths[7] = {1, 1, 1, 1, 1, 1, 1}, kHop = 3200;

static int load_weights(const char* path, uint64_t key) {
    std::ifstream in(path);
    if (!in) { fprintf(stderr, "enqueue_record: cannot read %s\n", path); return 1; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string name;
        if (!(ls >> name)) continue;
        std::vector<int64_t> shape;
        for (int64_t d; ls >> d;) shape.push_back(d);
        if (smtts_synth_tensor(H, name.c_str(), shape.data(), (int)shape.size(), ++key, 0.f, 0.05f)) return 1;
    }
    return 0;
}

static void operators(const Bufs& b, const std::string& cfgname) {
    void* const main2 = malloc(1);   // a second caller stream
    rec_names()[main2] = "main2";
    auto tag = [&](const std::string& s) { return s + " [" + cfgname + "]"; };

    // ---- 1. condition encoder: fork and join, and without a text half
    void* ws = dev<char>(smtts_cond_workspace_bytes(H, B, R, P));
    call(tag("cond_encode B2 R3 P5"), [&] {
        return smtts_cond_encode(H, nullptr, b.ref, b.ref_len, b.ids, b.ph_mask, B, R, P, b.k_ref, b.v_ref, b.ref_mask, b.k_text, b.v_text, ws,
                                 smtts_cond_workspace_bytes(H, B, R, P), nullptr, nullptr);
    });
    call(tag("cond_encode B2 R3 P0"), [&] {
        return smtts_cond_encode(H, nullptr, b.ref, b.ref_len, nullptr, nullptr, B, R, 0, b.k_ref, b.v_ref, b.ref_mask, nullptr, nullptr, ws,
                                 smtts_cond_workspace_bytes(H, B, R, 0), nullptr, nullptr);
    });

    // ---- 2. one denoiser evaluation, and with the caller's rope table
    for (int rope = 0; rope < 2; ++rope) {
        const size_t n = smtts_denoise_workspace_bytes(H, B, 9, R, P);
        ws = dev<char>(n);
        call(tag(rope ? "denoise_step N9 rope" : "denoise_step N9"), [&] {
            return smtts_denoise_step(H, nullptr, b.x, b.mask, b.t, b.k_ref, b.v_ref, b.ref_mask, b.k_text, b.v_text, b.ph_mask,
                                      rope ? b.rope : nullptr, B, 9, R, P, b.v, ws, n);
        });
    }

    // ---- 3.-9. the samplers
    struct S {
        const char* what; void* st = nullptr; int mode = 0, cfg = 0, N = 9; bool noise = false, steps = false;
        int tap = 0;   // 1: default tap, 2: explicit steps / layers / heads, 3: a tap that selects no layer
        int pinned = 0, start = 0, short_ws = 0;
    };
    auto sample = [&](const S& s) {
        const size_t n = smtts_sample_workspace_bytes(H, B, s.N, R, P, STEPS, s.cfg);
        void* const w = dev<char>(n);
        static const uint8_t tap_steps[STEPS] = {1, 0};
        call(tag(s.what), [&] {
            return smtts_sample_pinned(H, s.st, s.mode, STEPS, s.cfg, 1.5f, 0.5f, b.mask, b.k_ref, b.v_ref, b.ref_mask, b.k_text, b.v_text, b.ph_mask, B,
                                       s.N, R, P, s.noise ? b.noise : nullptr, 7, b.x, s.steps ? b.steps : nullptr, w, n - s.short_ws,
                                       s.tap == 2 ? tap_steps : nullptr, s.tap == 2 ? 0xa02u : s.tap == 3 ? 0u : 0xfffu, s.tap == 2 ? 0x24u : 0xffu,
                                       s.tap ? b.mass : nullptr, s.pinned ? b.x_pin : nullptr, s.pinned ? b.pin : nullptr, s.start);
        });
    };
    const char* const plain = "sample mode0 N9";
    S s;
    s.what = plain; sample(s);
    s = S(); s.what = "sample mode0 N9 noise steps_out"; s.noise = s.steps = true; sample(s);
    s = S(); s.what = "sample mode0 N9 on main2"; s.st = main2; sample(s);
    s = S(); s.what = "sample mode0 N8"; s.N = 8; sample(s);
    s = S(); s.what = "sample mode1 cfg1 N9"; s.mode = 1; s.cfg = 1; sample(s);
    s = S(); s.what = "sample mode1 cfg0 N9 steps_out"; s.mode = 1; s.steps = true; sample(s);
    s = S(); s.what = "sample_align default tap"; s.tap = 1; sample(s);
    s = S(); s.what = "sample_align steps 10 layers a02 heads 24"; s.tap = 2; sample(s);
    s = S(); s.what = "sample_pinned pins start_step 1"; s.pinned = 1; s.start = 1; s.noise = true; sample(s);
    s = S(); s.what = "sample_pinned pins start_step 0 default tap"; s.pinned = 1; s.tap = 1; sample(s);
    s = S(); s.what = "refused: sample_pinned start_step == n_steps"; s.pinned = 1; s.start = STEPS; sample(s);
    s = S(); s.what = plain; sample(s);
    s = S(); s.what = "refused: sample_align tap without a layer"; s.tap = 3; sample(s);
    s = S(); s.what = plain; sample(s);
    s = S(); s.what = "refused: sample workspace one byte short"; s.short_ws = 1; sample(s);
    s = S(); s.what = plain; sample(s);

    // ---- 10. the stage hook: DiT embed / blocks / head over block ranges and paths, once and twice on its workspace; the encoders whole
    struct D { int net, what, l0, l1, path, rows, row0, rstride, rope; };
    static const D stages[] = {
        {0, 14, 0, 12, 0, B, 0, 1, 0}, {0, 15, 0, 12, 0, B, 0, 1, 0}, {0, 14, 0, 12, 1, 2, 1, 0, 1}, {0, 4, 3, 5, 0, B, 0, 1, 0},
        {0, 4, 3, 5, 1, 2, 1, 0, 0},   {0, 4, 3, 5, 2, B, 0, 1, 0},   {0, 4, 3, 5, 3, B, 0, 1, 1},   {0, 2, 0, 0, 0, 0, 0, 0, 0},
        {0, 8, 0, 0, 0, 0, 0, 0, 0},   {1, 15, 0, 12, 0, 0, 0, 0, 0}, {2, 15, 0, 8, 0, 0, 0, 0, 0},
    };
    for (const D& d : stages)
        for (int twice = 0; twice < 2; ++twice) {
            char what[128];
            snprintf(what, sizeof what, "test_dit_stage net%d what%d [%d,%d) path%d rows%d row0 %d rstride%d rope%d twice%d", d.net, d.what, d.l0,
                     d.l1, d.path, d.rows, d.row0, d.rstride, d.rope, twice);
            const int S_ = d.net == 1 ? R : d.net == 2 ? P : 9;
            call(tag(what), [&] {
                return smtts_test_dit_stage(H, nullptr, d.net, d.what, d.l0, d.l1, d.path, twice, d.net == 2 ? (const void*)b.ids : d.net == 1 ? (const void*)b.ref : (const void*)b.x,
                                            d.net == 1 ? b.ref_mask : d.net == 2 ? b.ph_mask : b.mask, B, S_, b.t, (d.what & 1) ? nullptr : b.mod, d.rows,
                                            d.row0, d.rstride, b.k_ref, b.v_ref, b.ref_mask, R, b.k_text, b.v_text, b.ph_mask, P,
                                            d.rope ? b.rope : nullptr, b.big[0], b.big[1], b.v, b.big[2], b.big[3], b.big[4], b.mod_out);
            });
        }

    // ---- 11. the codec: decode, encode, two consecutive streamed chunks on two slots, one stage of each half through the hook
    {
        float* const lat = dev<float>((size_t)B * 3 * 64);
        float* const audio = dev<float>((size_t)B * 3 * kHop);
        size_t n = smtts_decode_workspace_bytes(H, B, 3);
        ws = dev<char>(n);
        call(tag("codec_decode B2 T3"), [&] { return smtts_codec_decode(H, nullptr, lat, B, 3, audio, ws, n); });
        n = smtts_encode_workspace_bytes(H, B, kHop);
        ws = dev<char>(n);
        call(tag("codec_encode B2 one hop"), [&] { return smtts_codec_encode(H, nullptr, audio, B, kHop, lat, ws, n); });
        n = smtts_decode_stream_workspace_bytes(H, B, 2);
        ws = dev<char>(n);
        void* const pool = dev<char>(2 * smtts_decode_state_bytes(H));
        int64_t* const slots = dev<int64_t>(B);
        for (int chunk = 0; chunk < 2; ++chunk)
            call(tag(std::string("codec_decode_stream B2 T2 chunk") + char('0' + chunk)),
                 [&] { return smtts_codec_decode_stream(H, nullptr, lat, B, 2, pool, 2, slots, audio, ws, n); });
        // decoder stage 1 (C 512 -> 256, ratio 8) on 3 frames; encoder stage 6 (C 256 -> 512, stride 8) on 8: each one frame of the latent
        float* const sin_ = dev<float>((size_t)B * 8 * 512);
        float* const sout = dev<float>((size_t)B * 24 * 512);
        call(tag("test_codec_stage decoder stage1 what6 T3"), [&] { return smtts_test_codec_stage(H, nullptr, 1, 1, 2 | 4, sin_, B, 3, 512, sout, nullptr, nullptr); });
        call(tag("test_codec_stage encoder stage6 what6 T8"), [&] { return smtts_test_codec_stage(H, nullptr, 2, 6, 2 | 4, sin_, B, 8, 256, sout, nullptr, nullptr); });
    }

    // ---- 12. the scorers: the recogniser, the verifier at its smallest N and at two frame tiles, one call of each a byte short
    {
        float* const x = dev<float>((size_t)B * 70 * 64);
        int32_t* const n_len = dev<int32_t>(B);
        float* const logp = dev<float>((size_t)B * 4 * 5 * 198);
        float* const emb = dev<float>((size_t)B * 192);
        size_t n = smtts_asr_workspace_bytes(H, B, 5);
        ws = dev<char>(n);
        call(tag("asr_logprobs B2 N5"), [&] { return smtts_asr_logprobs(H, nullptr, x, n_len, B, 5, ws, n, logp); });
        call(tag("asr_logprobs B2 N5 workspace one byte short"), [&] { return smtts_asr_logprobs(H, nullptr, x, n_len, B, 5, ws, n - 1, logp); });
        for (int N : {6, 70}) {
            n = smtts_sv_workspace_bytes(H, B, N);
            ws = dev<char>(n);
            call(tag("sv_embed B2 N" + std::to_string(N)), [&] { return smtts_sv_embed(H, nullptr, x, n_len, B, N, ws, n, emb); });
        }
        call(tag("sv_embed B2 N70 workspace one byte short"), [&] { return smtts_sv_embed(H, nullptr, x, n_len, B, 70, ws, n - 1, emb); });
        // the tap hook: the same launches with a copy behind each, in front of them the fill of its own workspace
        size_t tb = smtts_test_scorer_tap_bytes(H, 0, B, 5, nullptr, 0);
        char* taps = dev<char>(tb);
        call(tag("test_scorer_taps asr B2 N5"), [&] { return smtts_test_scorer_taps(H, nullptr, 0, x, n_len, B, 5, logp, taps, tb); });
        call(tag("test_scorer_taps asr B2 N5 taps one byte short"), [&] { return smtts_test_scorer_taps(H, nullptr, 0, x, n_len, B, 5, logp, taps, tb - 1); });
        tb = smtts_test_scorer_tap_bytes(H, 1, B, 6, nullptr, 0);
        taps = dev<char>(tb);
        call(tag("test_scorer_taps sv B2 N6"), [&] { return smtts_test_scorer_taps(H, nullptr, 1, x, n_len, B, 6, emb, taps, tb); });
        call(tag("test_scorer_taps sv B2 N6 taps one byte short"), [&] { return smtts_test_scorer_taps(H, nullptr, 1, x, n_len, B, 6, emb, taps, tb - 1); });
    }
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: enqueue_record <DiT inventory> <codec, asr and sv inventory>\n"); return 2; }
    const Bufs b;
    for (int tuning = 0; tuning < 2; ++tuning)
        for (int preset : {2, 3}) {
            if (smtts_create(0, &H) || smtts_set_precision(H, preset) || smtts_set_tuning(H, tuning) ||
                smtts_set_codec_spec(H, 64, 8, 7, 4, 1e-5f, kRatios, 6, kDepths) || load_weights(argv[1], 0) || load_weights(argv[2], 1u << 20) ||
                smtts_finalize(H)) {
                fprintf(stderr, "enqueue_record: setup failed: %s\n", smtts_last_error(H));
                return 1;
            }
            operators(b, std::string(tuning ? "throughput " : "latency ") + (preset == 2 ? "f16" : "bf16x3"));
            smtts_destroy(H);
            H = nullptr;
            rec_forget();
        }
    for (void* p : g_dev) (void)hipFree(p);
    return 0;
}
