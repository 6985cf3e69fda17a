// Weight layouts of the latent scorers' kernels (asr.hip, sv.hip), as plain host functions over std::vector<float>: no HIP type, no
// Engine.  engine_scorers.hip reads a tensor back, packs it here and uploads the result; tests/host/scorer_pack_check.cpp holds the
// index math to a restatement of the layouts.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

// conv or linear weight (n_out, i_all, taps) row-major, input channels [0, i_use) -> 64 x 64 blocks [k][n] with k = tap * i_use + channel;
// block order: outputs outer, k inner; outputs rounded up to n_pad with zero columns.  i_use * taps and n_pad are multiples of 64.
inline std::vector<float> pack_blocks64(const std::vector<float>& w, long n_out, long i_all, long i_use, long taps, long n_pad) {
    std::vector<float> o((size_t)(n_pad * i_use * taps), 0.f);
    const long kb = taps * i_use / 64;
    for (long r = 0; r < n_out; ++r)
        for (long i = 0; i < i_use; ++i)
            for (long t = 0; t < taps; ++t) {
                const long k = t * i_use + i;
                o[(size_t)((((r / 64) * kb + k / 64) * 64 + k % 64) * 64 + r % 64)] = w[(size_t)((r * i_all + i) * taps + t)];
            }
    return o;
}

// columns [i0, i0 + i_use) of a k = 1 weight (n_out, i_all) -> [k][n_out]
inline std::vector<float> pack_cols(const std::vector<float>& w, long n_out, long i_all, long i0, long i_use) {
    std::vector<float> o((size_t)(n_out * i_use));
    for (long r = 0; r < n_out; ++r)
        for (long k = 0; k < i_use; ++k) o[(size_t)(k * n_out + r)] = w[(size_t)(r * i_all + i0 + k)];
    return o;
}

// BatchNorm1d in eval: y = (x - mean) / sqrt(var + 1e-5) * weight + bias = x * scale + shift.  false: a negative (or NaN) variance
inline bool fold_batchnorm(const std::vector<float>& weight, const std::vector<float>& bias, const std::vector<float>& mean,
                           const std::vector<float>& var, std::vector<float>& scale, std::vector<float>& shift) {
    scale.resize(weight.size());
    shift.resize(weight.size());
    for (size_t i = 0; i < weight.size(); ++i) {
        if (!(var[i] >= 0.f)) return false;
        const double s = (double)weight[i] / std::sqrt((double)var[i] + 1e-5);
        scale[i] = (float)s;
        shift[i] = (float)((double)bias[i] - (double)mean[i] * s);
    }
    return true;
}
