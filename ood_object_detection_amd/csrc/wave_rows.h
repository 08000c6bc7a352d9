// One row inside a wave, for the units that walk rows of class logits (or of channels) with one wave per row (logit_ood.hip,
// act_shaping.hip, energy_reg.hip).  A row of n elements is spread over the wave: lane t holds elements t, t + 64, ..
// in N registers, element j = lane + 64 i being live when j < n.  All 64 lanes call every routine here, with the same n; a sum
// runs over a lane's elements ascending and then over the lanes by the xor tree 32 .. 1 (wave_reduce_sum), so its bits depend on
// the row alone.  Which rows a unit reads is feature_rows.h's; the reductions of a workgroup and the compaction are compact.h's.
#pragma once
#include <type_traits>
#include "common.h"
#include "compact.h"
#include "feature_rows.h"                                       // fo_ld

namespace {

constexpr int WR_NONE = 0x7FFFFFFF;                             // the argmax of a row in which nothing equals the maximum (a NaN row)

DEV int wr_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}

// the row at p (float32, or bfloat16 widened exactly); 0 beyond n
template <int N> DEV void wr_load(const char* p, int n, int bf16, int lane, float (&z)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = lane + 64 * i < n ? fo_ld(p, lane + 64 * i, bf16) : 0.f;
}

// the maximum and (*kstar) the lowest index that holds it, WR_NONE when none does: the caller tests 0 <= *kstar < n
template <int N> DEV float wr_argmax(const float (&z)[N], int n, int lane, int* kstar) {
    float m = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (lane + 64 * i < n) m = fmaxf(m, z[i]);
    m = wave_reduce_max(m);
    int ks = WR_NONE;
#pragma unroll
    for (int i = N - 1; i >= 0; --i)
        if (lane + 64 * i < n && z[i] == m) ks = lane + 64 * i;
    *kstar = wr_min(ks);
    return m;
}

// bit i of the result: element lane + 64 i is among the k largest by key (fo_key of the value's bits, formed by the caller; equal
// keys: the lower index first).  A 32-step search on the keys with ballots, then the ties ranked in index order; a register with
// no live element in any lane takes no part.
template <int N> DEV unsigned wr_top(const unsigned (&key)[N], int n, int k, int lane) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) all |= (lane + 64 * i < n ? 1u : 0u) << i;
    if (k >= n) return all;
    unsigned tau = 0;                                           // the largest t with at least k keys >= t: the k-th largest key
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = tau | (1u << bit);
        unsigned c = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (64 * i < n) c += fo_popc(__ballot(((all >> i) & 1u) && key[i] >= cand));
        if (c >= (unsigned)k) tau = cand;
    }
    unsigned above = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (64 * i < n) above += fo_popc(__ballot(((all >> i) & 1u) && key[i] > tau));
    const unsigned need = (unsigned)k - above;                  // of the keys equal to tau, in index order
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned sel = 0, run = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (64 * i < n) {
            const bool live = (all >> i) & 1u, tie = live && key[i] == tau;
            const unsigned long long bal = __ballot(tie);
            const unsigned rank = run + fo_popc(bal & below);
            run += fo_popc(bal);
            if (live && (key[i] > tau || (tie && rank < need))) sel |= 1u << i;
        }
    }
    return sel;
}

// the log-sum-exp of u = z / T in its pieces, from mz = max z: *m = mz / T (= max u: the division is monotone) and
// *s = sum exp(z_k / T - *m); the log-sum-exp is *m + log *s
template <int N> DEV void wr_lse(const float (&z)[N], int n, float T, float mz, int lane, float* m, float* s) {
    const float mu = mz / T;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) t += lane + 64 * i < n ? expf(z[i] / T - mu) : 0.f;
    *m = mu; *s = wave_reduce_sum(t);
}

DEV float wr_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// ---- host ----
// fn(std::integral_constant<int, NC>{}) for the registers a lane needs for C classes.  The steps are multiples of 16, so C and C
// rounded up to 16 choose the same.
template <typename Fn> void wr_for_classes(int C, Fn fn) {
    if (C <= 128) fn(std::integral_constant<int, 2>{});
    else if (C <= 256) fn(std::integral_constant<int, 4>{});
    else if (C <= 512) fn(std::integral_constant<int, 8>{});
    else fn(std::integral_constant<int, 16>{});
}

}  // namespace
