// Stand-alone check program of smalltts_amd/csrc/scorer_pack.hpp (tests/test_scorer_pack_cpu.py): host compiler, no HIP.
//   scorer_pack_check blocks n_out i_all i_use taps n_pad   packs the index-valued weight w[i] = i, prints the packed values
//   scorer_pack_check cols n_out i_all i0 i_use             the same for pack_cols
//   scorer_pack_check bn n                                  reads weight, bias, mean, var (n float32 bit patterns each, hex) from stdin,
//                                                           prints "ok" and the bit patterns of scale and shift, or "refused"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../smalltts_amd/csrc/scorer_pack.hpp"

static std::vector<float> iota(long n) {
    std::vector<float> w((size_t)n);
    for (long i = 0; i < n; ++i) w[(size_t)i] = (float)i;
    return w;
}

static void print_ints(const std::vector<float>& v) {
    for (float x : v) printf("%ld\n", (long)x);
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    auto arg = [&](int i) { return atol(argv[i]); };
    if (what == "blocks" && argc == 7) {
        print_ints(pack_blocks64(iota(arg(2) * arg(3) * arg(5)), arg(2), arg(3), arg(4), arg(5), arg(6)));
    } else if (what == "cols" && argc == 6) {
        print_ints(pack_cols(iota(arg(2) * arg(3)), arg(2), arg(3), arg(4), arg(5)));
    } else if (what == "bn" && argc == 3) {
        const long n = arg(2);
        std::vector<float> in[4], scale, shift;
        for (auto& v : in)
            for (long i = 0; i < n; ++i) {
                uint32_t bits;
                if (scanf("%" SCNx32, &bits) != 1) { fprintf(stderr, "scorer_pack_check: short input\n"); return 2; }
                float f;
                memcpy(&f, &bits, 4);
                v.push_back(f);
            }
        if (!fold_batchnorm(in[0], in[1], in[2], in[3], scale, shift)) { printf("refused\n"); return 0; }
        printf("ok\n");
        for (const auto* v : {&scale, &shift})
            for (float f : *v) {
                uint32_t bits;
                memcpy(&bits, &f, 4);
                printf("%08" PRIx32 "\n", bits);
            }
    } else {
        fprintf(stderr, "usage: scorer_pack_check blocks|cols|bn ...\n");
        return 2;
    }
    return 0;
}
