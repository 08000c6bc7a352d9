// What the episode loss kernels (episode_loss.hip, episode_support.hip) share: the limits, the index clamp and the wave's row load.
#pragma once
#include "common.h"

namespace {

constexpr int PL_MAX_DL = 8;              // d <= 64 * PL_MAX_DL
constexpr int PL_MAX_M = 64;
constexpr int PL_MAX_G = 1024;
constexpr int PL_MAX_PARTS = 32;

DEV long long pl_clamp(long long v, long long hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

// the row in the lanes' registers (column lane + 64 k), returns 1 / max(||row||, 1e-12): the sum episode_prep_kernel forms
DEV float pl_load_row(const float* row, int d, int lane, float (&v)[PL_MAX_DL]) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) { const int c = lane + 64 * k; v[k] = c < d ? row[c] : 0.f; }
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) ss += v[k] * v[k];
    ss = wave_reduce_sum(ss);
    return 1.0f / fmaxf(sqrtf(ss), 1e-12f);
}

inline bool pl_shape_ok(int n, int d, int m) {
    return n > 0 && d > 0 && m > 0 && m <= PL_MAX_M && d <= 64 * PL_MAX_DL && (long long)m * d <= 16384 && n >= m;
}

}  // namespace
