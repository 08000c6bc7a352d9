// Activation-shaping OOD scores on the device: ReAct (Sun et al. 2021), ASH-P / ASH-B / ASH-S (Djurisic et al. 2023), SCALE (Xu et al.
// 2024) and GradNorm (Huang et al. 2021) from the class head's penultimate activation - the output of the depthwise 3 x 3 of
// class_net.predict - recomputed from the class tower, shaped, and multiplied with the pointwise weight again.  DICE
// (Sun & Li 2022) is a mask on that weight and so host glue (ood_shaping.py).
//
//   penultimate row of a cell, float32 (bfloat16 widened exactly), one rounding per operation:
//     d_j = t_0j x_0j,  then d_j = d_j + t_kj x_kj for k = 1 .. 8;  x_k: the tower value at (y + ky - 1, x + kx - 1), k = 3 ky + kx,
//     0 outside the map (the product with 0 and the sum are still taken, so the bits are those of the plain restatement)
//   shaping d -> x':  none x' = d;  react x'_j = min(d_j, c), c read from device memory;  with the kept set = the k largest d_j by
//     value (-0 = +0; equal values: the lower j first), s1 = sum_j max(d_j, 0), s2 = the same sum over the kept set,
//     f = exp(s1 / s2) (1 where s2 == 0):  ash_p kept d_j, others 0;  ash_b kept s1 / k, others 0;  ash_s kept d_j f, others 0;
//     scale d_j f for every j.  s1 and s2: lane t adds its channels t, t + 64, .. ascending, then the xor tree 32 .. 1 - an order that
//     depends on the row alone.  The selection is a 32-step search on the ordered bit patterns with ballots.
//   logits of anchor slot a: z_c = bias[a][c] + sum_j W[a C + c][j] x'_j;  u = z / T;  energy = -(T * (max u + log sum exp(u - max u)));
//     max_logit = max z;  class = the lowest argmax of z;  gradnorm = (sum_c |p_c - 1 / C|) * (sum_j |d_j|) with p the softmax at
//     T = 1 of the logits of the UNSHAPED row d.  A row with a non-finite d_j scores NaN, NaN, -1, NaN.
//
//   score        one wave per [B, K] entry, four a workgroup: d and x' in the wave's LDS, lane t holds classes t, t + 64, ..; the
//                weight is read transposed ([A][F][Cp]) so that lanes read consecutive addresses; sum_j is a float64 fma chain, j ascending,
//                rounded to float32 once.
//   score_cells  16 cells per workgroup: each wave forms the shaped rows of four of them ONCE, then wave w takes anchor slots
//                w, w + 4, ..: the [16 x Fp] by [Fp x Cp] product runs on the float32-input MFMA (16x16x4) a class tile at a time (K-chunk c of 16
//                into accumulator c mod 4, then (a0 + a1) + (a2 + a3)),
//                the log-sum-exp is kept online in registers per (row, lane) over the tiles ascending and then combined over the 16
//                lanes of a row by the xor tree 1 .. 8; the A * C logits are never stored.  gradnorm takes two more products of the
//                unshaped rows.  A cell's bits depend on nothing but the cell: not on its place in a workgroup, nor on the call.
//   A row's scores are NOT bit-equal between the two forms (float64 chain against float32 MFMA tiles, two-pass against online log-sum-exp).
//   fit          per entry d, a flag (counts and finite) and the histogram of the upper 16 key bits of every d_j (integer atomics);
//                the flagged entries compacted in (b, j) order (compact.h); workgroup s of 256 adds the rows of chunk s of that list
//                to float64 partials - wave w rows w, w + 4, .. in list order, then the waves in order -; one workgroup adds the chunks
//                in chunk order onto sum_d and the number of rows onto n.  The chunk bounds follow from the number of flagged rows alone.
//
// Every row and neighbour index is compared with its extent before a pointer is formed, every store index before the store; no call
// synchronises with the host or allocates, so all of them can be captured in a graph.
#include "common.h"
#include "feature_rows.h"
#include "wave_rows.h"

namespace {

constexpr int AS_MAX_CLASSES = 1024;
constexpr int AS_WAVES = 4;
constexpr int AS_CELLS = 16;                                     // cells of a score_cells workgroup
constexpr int AS_CHUNKS = 256;                                   // row chunks of the fit partials
enum { AS_M_NONE = 0, AS_M_REACT, AS_M_ASH_P, AS_M_ASH_B, AS_M_ASH_S, AS_M_SCALE, AS_METHODS };

struct AsLevels { FoLevels L; int h[FO_MAX_LEVELS], w[FO_MAX_LEVELS]; };

struct AsArgs {
    AsLevels T; FoSel sel;
    int F, C, Cp, A;
    const float *taps, *w_rows, *w_tiles, *bias;                // [9][F], [A][F][Cp], [A][Cp][Fp], [A][Cp]
    int method, k; const float* react_c; float temp;
    float *energy, *max_logit; long long* cls; float *gradnorm, *rows;
    int* flag; unsigned *list, *counts, *header; unsigned nblocks;
    double* partial; long long* n; double* sum_d; unsigned long long* hist;
};

DEV float as_nan() { return __uint_as_float(0x7FC00000u); }
DEV bool as_finite(float v) { return v - v == 0.f; }
// the ordered key of a value, -0 as +0
DEV unsigned as_key(float v) { return fo_key(v == 0.f ? 0u : __float_as_uint(v)); }

// d of cell `cell` (< P) of image b: lane t holds channels t + 64 i.  False when some d_j is not finite.
template <int NV> DEV bool as_dw(const AsLevels& T, const float* taps, int F, unsigned b, unsigned cell, int lane, float (&d)[NV]) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < FO_MAX_LEVELS; ++k) l += (k < T.L.n && cell >= T.L.start[k]) ? 1 : 0;
    int h = 1, w = 1;
#pragma unroll
    for (int k = 0; k < FO_MAX_LEVELS; ++k)
        if (k == l) { h = T.h[k]; w = T.w[k]; }
    const int local = (int)(cell - T.L.start[l]);
    const int y = local / w, x = local - y * w;
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
        const int ny = y + k / 3 - 1, nx = x + k % 3 - 1;
        const bool inside = ny >= 0 && ny < h && nx >= 0 && nx < w;
        const char* p = inside ? fo_row(T.L, b, T.L.start[l] + (unsigned)(ny * w + nx)) : nullptr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int j = lane + 64 * i;
            float v = 0.f;
            if (j < F) {
                const float xv = p ? fo_ld(p, j, T.L.bf16) : 0.f;
                const float pr = taps[k * F + j] * xv;
                v = k == 0 ? pr : d[i] + pr;
            }
            d[i] = v;
        }
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) bad = bad || !as_finite(d[i]);
    return __ballot(bad) == 0ull;
}

// d -> x' (zero beyond F)
template <int NV> DEV void as_shape(const AsArgs& a, const float (&d)[NV], int lane, float (&x)[NV]) {
    const int F = a.F, method = a.method;
    if (method == AS_M_NONE || method == AS_M_REACT) {
        const float c = method == AS_M_REACT ? a.react_c[0] : 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) x[i] = lane + 64 * i < F ? (method == AS_M_REACT ? fminf(d[i], c) : d[i]) : 0.f;
        return;
    }
    unsigned key[NV];                                           // the k largest d by value, equal values: the lower channel first
#pragma unroll
    for (int i = 0; i < NV; ++i) key[i] = as_key(d[i]);
    const unsigned kept = wr_top<NV>(key, F, a.k, lane);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float pos = lane + 64 * i < F ? fmaxf(d[i], 0.f) : 0.f;
        s1 += pos;
        s2 += ((kept >> i) & 1u) ? pos : 0.f;
    }
    s1 = wave_reduce_sum(s1);
    s2 = wave_reduce_sum(s2);
    const float f = s2 == 0.f ? 1.f : expf(s1 / s2);
    const float even = s1 / (float)a.k;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool live = lane + 64 * i < F, kp = (kept >> i) & 1u;
        float v;
        if (method == AS_M_ASH_P) v = kp ? d[i] : 0.f;
        else if (method == AS_M_ASH_B) v = kp ? even : 0.f;
        else if (method == AS_M_ASH_S) v = kp ? d[i] * f : 0.f;
        else v = d[i] * f;
        x[i] = live ? v : 0.f;
    }
}

template <int NV> DEV float as_l1(const float (&d)[NV]) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) t += fabsf(d[i]);              // (0 beyond F)
    return wave_reduce_sum(t);
}

// ---- entries form ------------------------------------------------------------------------------------------------------------
// z_c = bias_c + sum_j W[j][c] x_j of the wave's row x (LDS), lane t: classes t + 64 m; 0 beyond C.  The sum is a float64 fma chain, j
// ascending, rounded to float32 once: the entries form pays a few thousand rows for it, and its logits are then correctly rounded
// but for the bias sum
template <int NC> DEV void as_logits(const float* x, const float* W, const float* bias, int F, int C, int Cp, int lane, float (&z)[NC]) {
    double acc[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = 0.0;
    for (int j = 0; j < F; ++j) {
        const double xv = (double)x[j];
#pragma unroll
        for (int m = 0; m < NC; ++m) {
            const int c = lane + 64 * m;
            if (c < C) acc[m] = fma((double)W[(long long)j * Cp + c], xv, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) z[m] = lane + 64 * m < C ? bias[lane + 64 * m] + (float)acc[m] : 0.f;
}

// max u + log sum exp(u - max u) of u = z / T, max z and its lowest argmax
template <int NC> DEV float as_lse(const float (&z)[NC], int C, float T, int lane, float* maxz, int* kstar) {
    float mu, s;
    *maxz = wr_argmax<NC>(z, C, lane, kstar);
    wr_lse<NC>(z, C, T, *maxz, lane, &mu, &s);
    return mu + logf(s);
}

template <int NT, int NC>
__global__ __launch_bounds__(AS_WAVES * 64) void as_score_kernel(AsArgs a) {
    constexpr int FP = 16 * NT, NV = (FP + 63) / 64;
    __shared__ float xs[AS_WAVES][2][FP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned i = (unsigned)blockIdx.x * AS_WAVES + wave;  // the same for the whole wave
    const int F = a.F, C = a.C;
    unsigned b = 0; long long an = 0;
    int state = 0, slot = 0;                                    // 0: the entry does not count, 1: scored, 2: a non-finite d
    float d[NV], x[NV], l1 = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) { d[q] = 0.f; x[q] = 0.f; }
    if (fo_select(a.sel, i, &b, &an)) {
        slot = (int)(an % a.A);
        const bool fin = as_dw<NV>(a.T, a.taps, F, b, (unsigned)(an / a.A), lane, d);
        state = fin ? 1 : 2;
        if (fin) { as_shape<NV>(a, d, lane, x); l1 = as_l1<NV>(d); }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const int j = lane + 64 * q;
        if (j < FP) { xs[wave][0][j] = state == 1 ? x[q] : 0.f; xs[wave][1][j] = state == 1 ? d[q] : 0.f; }
        if (a.rows && i < a.sel.total && j < F) a.rows[(long long)i * F + j] = state == 1 ? x[q] : (state == 2 ? as_nan() : 0.f);
    }
    __syncthreads();
    if (i >= a.sel.total) return;
    if (state != 1) {
        if (lane == 0) {
            const float v = state == 2 ? as_nan() : 0.f;
            a.energy[i] = v; a.max_logit[i] = v; a.cls[i] = -1;
            if (a.gradnorm) a.gradnorm[i] = v;
        }
        return;
    }
    const float* W = a.w_rows + (long long)slot * F * a.Cp;
    const float* bias = a.bias + (long long)slot * a.Cp;
    float z[NC], mz; int ks;
    as_logits<NC>(xs[wave][0], W, bias, F, C, a.Cp, lane, z);
    const float lse = as_lse<NC>(z, C, a.temp, lane, &mz, &ks);
    if (lane == 0) {
        a.energy[i] = -(a.temp * lse);
        a.max_logit[i] = mz;
        a.cls[i] = ks >= 0 && ks < C ? (long long)ks : -1;
    }
    if (!a.gradnorm) return;
    as_logits<NC>(xs[wave][1], W, bias, F, C, a.Cp, lane, z);
    const float lse1 = as_lse<NC>(z, C, 1.f, lane, &mz, &ks);
    const float invc = 1.f / (float)C;
    float g = 0.f;
#pragma unroll
    for (int m = 0; m < NC; ++m) g += lane + 64 * m < C ? fabsf(expf(z[m] - lse1) - invc) : 0.f;
    g = wave_reduce_sum(g);
    if (lane == 0) a.gradnorm[i] = g * l1;
}

// ---- cells form --------------------------------------------------------------------------------------------------------------
// fn(q, c, z): logit z of row 4 (lane >> 4) + q and class c = 16 tile + (lane & 15) of one anchor slot, the tiles ascending
template <int NT, typename Fn> DEV void as_tiles(const float* xs, const float* W, const float* bias, int Cp, int r16, int g, Fn fn) {
    constexpr int FP = 16 * NT, PITCH = FP + 4;
#pragma unroll 1
    for (int tile = 0; tile < Cp / 16; ++tile) {
        f32x4 acc[4];                                           // K-chunk c goes to accumulator c mod 4: four short chains, then a tree
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* wr = W + (long long)(tile * 16 + r16) * FP + g * 4;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const Frag<float> fa = ld_frag<float>(xs + r16 * PITCH + 16 * c + g * 4);
            const Frag<float> fb = ld_frag<float>(wr + 16 * c);
            mma_chunk(fa, fb, acc[c & 3]);
        }
        const float bv = bias[tile * 16 + r16];
#pragma unroll
        for (int q = 0; q < 4; ++q) fn(q, tile * 16 + r16, bv + ((acc[0][q] + acc[1][q]) + (acc[2][q] + acc[3][q])));
    }
}

// the log-sum-exp of u = z / T (*lse), max z (*bz) and its lowest argmax (*bc) of the four rows of a lane's group, every lane of the
// group holding the result
template <int NT> DEV void as_cells_lse(const float* xs, const float* W, const float* bias, int C, int Cp, float T, int r16, int g,
                                        float (&lse)[4], float (&bz)[4], int (&bc)[4]) {
    float m[4], s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { m[q] = -__builtin_inff(); s[q] = 0.f; bz[q] = -__builtin_inff(); bc[q] = WR_NONE; }
    as_tiles<NT>(xs, W, bias, Cp, r16, g, [&](int q, int c, float z) {
        if (c >= C) return;                                     // (the padding: bias -inf)
        const float u = z / T;
        if (u > m[q]) { s[q] = s[q] * expf(m[q] - u) + 1.f; m[q] = u; }
        else s[q] += expf(u - m[q]);
        if (z > bz[q]) { bz[q] = z; bc[q] = c; }                // classes ascending: the lowest argmax stays
    });
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float om = __shfl_xor(m[q], o, 64), os = __shfl_xor(s[q], o, 64), oz = __shfl_xor(bz[q], o, 64);
            const int oc = __shfl_xor(bc[q], o, 64);
            const float mm = fmaxf(m[q], om);
            const float wa = m[q] == mm ? 1.f : expf(m[q] - mm), wb = om == mm ? 1.f : expf(om - mm);
            s[q] = s[q] * wa + os * wb;                         // (a product and a sum on both sides of the exchange: the same bits)
            m[q] = mm;
            if (oz > bz[q] || (oz == bz[q] && oc < bc[q])) { bz[q] = oz; bc[q] = oc; }
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) lse[q] = m[q] + logf(s[q]);
}

template <int NT>
__global__ __launch_bounds__(AS_WAVES * 64) void as_cells_kernel(AsArgs a) {
    constexpr int FP = 16 * NT, PITCH = FP + 4, NV = (FP + 63) / 64;
    __shared__ __attribute__((aligned(16))) float xs[AS_CELLS * PITCH], ds[AS_CELLS * PITCH];
    __shared__ float l1s[AS_CELLS];
    __shared__ int rv[AS_CELLS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r16 = lane & 15, g = lane >> 4;
    const int F = a.F, C = a.C, A = a.A;
    const unsigned P = a.T.L.P, total = a.sel.total;            // total = B * P cells
    const unsigned row0 = (unsigned)blockIdx.x * AS_CELLS;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const unsigned ci = row0 + r;                           // the same for the whole wave
        int state = 0;
        float d[NV], x[NV], l1 = 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q) { d[q] = 0.f; x[q] = 0.f; }
        if (ci < total) {
            const unsigned b = ci / P;
            const bool fin = as_dw<NV>(a.T, a.taps, F, b, ci - b * P, lane, d);
            state = fin ? 1 : 2;
            if (fin) { as_shape<NV>(a, d, lane, x); l1 = as_l1<NV>(d); }
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int j = lane + 64 * q;
            if (j < FP) { xs[r * PITCH + j] = state == 1 ? x[q] : 0.f; ds[r * PITCH + j] = state == 1 ? d[q] : 0.f; }
        }
        if (lane == 0) { rv[r] = state; l1s[r] = l1; }
    }
    __syncthreads();
    const long long N = (long long)A * P;
    const float invc = 1.f / (float)C;
#pragma unroll 1
    for (int slot = wave; slot < A; slot += AS_WAVES) {
        const float* W = a.w_tiles + (long long)slot * a.Cp * FP;
        const float* bias = a.bias + (long long)slot * a.Cp;
        float lse[4], bz[4], gn[4]; int bc[4];
        as_cells_lse<NT>(xs, W, bias, C, a.Cp, a.temp, r16, g, lse, bz, bc);
        if (a.gradnorm) {
            float lse1[4], bz1[4]; int bc1[4];
            as_cells_lse<NT>(ds, W, bias, C, a.Cp, 1.f, r16, g, lse1, bz1, bc1);
#pragma unroll
            for (int q = 0; q < 4; ++q) gn[q] = 0.f;
            as_tiles<NT>(ds, W, bias, a.Cp, r16, g, [&](int q, int c, float z) {
                if (c < C) gn[q] += fabsf(expf(z - lse1[q]) - invc);
            });
#pragma unroll
            for (int o = 1; o < 16; o <<= 1)
#pragma unroll
                for (int q = 0; q < 4; ++q) gn[q] += __shfl_xor(gn[q], o, 64);
        }
        if (r16 == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * g + q;
                const unsigned ci = row0 + r;
                if (ci >= total) continue;
                const unsigned b = ci / P;
                const long long at = (long long)b * N + (long long)(ci - b * P) * A + slot;
                const bool ok = rv[r] == 1;
                a.energy[at] = ok ? -(a.temp * lse[q]) : as_nan();
                a.max_logit[at] = ok ? bz[q] : as_nan();
                a.cls[at] = ok && bc[q] >= 0 && bc[q] < C ? (long long)bc[q] : -1;
                if (a.gradnorm) a.gradnorm[at] = ok ? gn[q] * l1s[r] : as_nan();
            }
        }
    }
}

// ---- fit ---------------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(AS_WAVES * 64) void as_fit_rows_kernel(AsArgs a) {
    constexpr int NV = (16 * NT + 63) / 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned i = (unsigned)blockIdx.x * AS_WAVES + wave;
    if (i >= a.sel.total) return;
    unsigned b; long long an;
    bool keep = false;
    if (fo_select(a.sel, i, &b, &an)) {
        float d[NV];
        keep = as_dw<NV>(a.T, a.taps, a.F, b, (unsigned)(an / a.A), lane, d);
        if (keep) {
#pragma unroll
            for (int q = 0; q < NV; ++q)
                if (lane + 64 * q < a.F) atomicAdd(a.hist + (fo_key(__float_as_uint(d[q])) >> 16), 1ull);
        }
    }
    if (lane == 0) a.flag[i] = keep ? 1 : 0;
}

DEV bool cp_keep(const AsArgs& a, unsigned i) { return i < a.sel.total && a.flag[i] != 0; }
DEV unsigned cp_begin(const AsArgs&) { return 0u; }
DEV void cp_finish(const AsArgs& a, unsigned, unsigned total) { a.header[0] = fo_min(total, a.sel.total); }

// workgroup s: partial[s][j] = sum of d_j over the rows of chunk s of the compacted list
template <int NT>
__global__ __launch_bounds__(AS_WAVES * 64) void as_fit_sum_kernel(AsArgs a) {
    constexpr int FP = 16 * NT, NV = (FP + 63) / 64;
    __shared__ double part[AS_WAVES][FP];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned V = fo_min(a.header[0], a.sel.total);
    const unsigned len = (V + AS_CHUNKS - 1) / AS_CHUNKS;
    const unsigned lo = fo_min((unsigned)blockIdx.x * len, V), hi = fo_min(lo + len, V);
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    for (unsigned v = lo + wave; v < hi; v += AS_WAVES) {
        const unsigned i = a.list[v];                           // the same for the whole wave
        unsigned b; long long an;
        if (!fo_select(a.sel, i, &b, &an)) continue;
        float d[NV];
        if (!as_dw<NV>(a.T, a.taps, a.F, b, (unsigned)(an / a.A), lane, d)) continue;
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] += (double)d[q];
    }
#pragma unroll
    for (int q = 0; q < NV; ++q)
        if (lane + 64 * q < FP) part[wave][lane + 64 * q] = acc[q];
    __syncthreads();
    for (int j = threadIdx.x; j < a.F; j += AS_WAVES * 64) {
        double t = part[0][j];
        for (int w = 1; w < AS_WAVES; ++w) t += part[w][j];
        a.partial[(long long)blockIdx.x * a.F + j] = t;
    }
}

// one workgroup: the chunks in chunk order, then onto the running statistics
__global__ __launch_bounds__(256) void as_fit_reduce_kernel(AsArgs a) {
    for (int j = threadIdx.x; j < a.F; j += 256) {
        double t = 0.0;
        for (int s = 0; s < AS_CHUNKS; ++s) t += a.partial[(long long)s * a.F + j];
        a.sum_d[j] += t;
    }
    if (threadIdx.x == 0) a.n[0] += (long long)fo_min(a.header[0], a.sel.total);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct AsLayout { long long flag, list, counts, header, partial, bytes; unsigned nblocks; };

bool as_layout(long long rows, int F, AsLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS || !fo_width_ok(F)) return false;
    L->nblocks = (unsigned)((rows + FO_TILE - 1) / FO_TILE);
    FoCarve ws;
    L->flag = ws.take(rows * 4);
    L->list = ws.take(rows * 4);
    L->counts = ws.take((long long)L->nblocks * 4);
    L->header = ws.take(256);
    L->partial = ws.take((long long)AS_CHUNKS * F * 8);
    L->bytes = ws.at;
    return true;
}

// heights and widths of the levels beside the table; false: refuse
bool as_levels(const int* heights, const int* widths, int num_levels, const long long* cells, AsLevels* T) {
    if (!heights || !widths) return false;
    for (int l = 0; l < FO_MAX_LEVELS; ++l) { T->h[l] = 1; T->w[l] = 1; }
    for (int l = 0; l < num_levels; ++l) {
        if (heights[l] < 1 || widths[l] < 1 || (long long)heights[l] * widths[l] != cells[l]) return false;
        T->h[l] = heights[l]; T->w[l] = widths[l];
    }
    return true;
}

bool as_method(int method, int k, int F, const float* react_c, float temperature) {
    if (method < 0 || method >= AS_METHODS) return false;
    if (method == AS_M_REACT && !react_c) return false;
    if (method >= AS_M_ASH_P && (k < 1 || k > F)) return false;
    return temperature > 0.f && temperature < __builtin_inff();
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_act_shaping_workspace_bytes(long long rows, int F) {
    AsLayout L;
    return as_layout(rows, F, &L) ? L.bytes : EFFDET_EINVAL;
}

extern "C" int effdet_act_shaping_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                        const long long* level_batch_strides, const long long* level_cell_strides,
                                        const long long* level_channel_strides, const int* level_heights, const int* level_widths, int F,
                                        int C, int A, int B, long long K, const long long* anchor_index, const void* count,
                                        int count_is_int64, const float* taps, const float* w_rows, const float* bias, int method, int k,
                                        const float* react_c, float temperature, float* energy, float* max_logit,
                                        long long* predicted_class, float* gradnorm, float* rows) {
    AsArgs a = AsArgs{};
    if (!fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.T.L, &a.sel))
        return EFFDET_EINVAL;
    if (!as_levels(level_heights, level_widths, num_levels, level_cells, &a.T)) return EFFDET_EINVAL;
    if (C < 1 || C > AS_MAX_CLASSES || !as_method(method, k, F, react_c, temperature)) return EFFDET_EINVAL;
    if (!taps || !w_rows || !bias || !energy || !max_logit || !predicted_class) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    a.F = F; a.C = C; a.Cp = (C + 15) / 16 * 16; a.A = A;
    a.taps = taps; a.w_rows = w_rows; a.bias = bias;
    a.method = method; a.k = k; a.react_c = react_c; a.temp = temperature;
    a.energy = energy; a.max_logit = max_logit; a.cls = predicted_class; a.gradnorm = gradnorm; a.rows = rows;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a.sel.total + AS_WAVES - 1) / AS_WAVES), block(AS_WAVES * 64);
    fo_for_width(F, [&](auto nt) {
        wr_for_classes(a.Cp, [&](auto nc) {
            hipLaunchKernelGGL((as_score_kernel<decltype(nt)::value, decltype(nc)::value>), grid, block, 0, st, a);
        });
    });
    return effdet_check_launch();
}

extern "C" int effdet_act_shaping_score_cells(void* stream, int dtype, int num_levels, const void* const* level_bases,
                                              const long long* level_cells, const long long* level_batch_strides,
                                              const long long* level_cell_strides, const long long* level_channel_strides,
                                              const int* level_heights, const int* level_widths, int F, int C, int A, int B,
                                              const float* taps, const float* w_tiles, const float* bias, int method, int k,
                                              const float* react_c, float temperature, float* energy, float* max_logit,
                                              long long* predicted_class, float* gradnorm) {
    AsArgs a = AsArgs{};
    if (!fo_width_ok(F) || A < 1 || A > (1 << 20) ||
        !fo_levels(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, B, &a.T.L))
        return EFFDET_EINVAL;
    if (!as_levels(level_heights, level_widths, num_levels, level_cells, &a.T)) return EFFDET_EINVAL;
    if (C < 1 || C > AS_MAX_CLASSES || !as_method(method, k, F, react_c, temperature)) return EFFDET_EINVAL;
    if (!taps || !w_tiles || !bias || !energy || !max_logit || !predicted_class) return EFFDET_EINVAL;
    EFFDET_ENTER();
    a.sel = FoSel{};
    a.sel.total = (unsigned)((long long)B * a.T.L.P);            // cells of the call (<= 2^31: fo_levels)
    a.F = F; a.C = C; a.Cp = (C + 15) / 16 * 16; a.A = A;
    a.taps = taps; a.w_tiles = w_tiles; a.bias = bias;
    a.method = method; a.k = k; a.react_c = react_c; a.temp = temperature;
    a.energy = energy; a.max_logit = max_logit; a.cls = predicted_class; a.gradnorm = gradnorm;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long long)a.sel.total + AS_CELLS - 1) / AS_CELLS)), block(AS_WAVES * 64);
    fo_for_width(F, [&](auto nt) { hipLaunchKernelGGL(as_cells_kernel<decltype(nt)::value>, grid, block, 0, st, a); });
    return effdet_check_launch();
}

extern "C" int effdet_act_shaping_fit(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                      const long long* level_batch_strides, const long long* level_cell_strides,
                                      const long long* level_channel_strides, const int* level_heights, const int* level_widths, int F,
                                      int A, int B, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                                      const float* taps, long long* n, double* sum_d, long long* hist, void* workspace,
                                      long long workspace_bytes) {
    AsArgs a = AsArgs{};
    if (!fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.T.L, &a.sel))
        return EFFDET_EINVAL;
    if (!as_levels(level_heights, level_widths, num_levels, level_cells, &a.T)) return EFFDET_EINVAL;
    AsLayout L;
    if (!as_layout((long long)B * K, F, &L)) return EFFDET_EINVAL;
    if (!taps || !n || !sum_d || !hist || !workspace || workspace_bytes < L.bytes) return EFFDET_EINVAL;
    EFFDET_ENTER();
    char* ws = reinterpret_cast<char*>(workspace);
    a.F = F; a.A = A; a.taps = taps;
    a.flag = reinterpret_cast<int*>(ws + L.flag); a.list = reinterpret_cast<unsigned*>(ws + L.list);
    a.counts = reinterpret_cast<unsigned*>(ws + L.counts); a.header = reinterpret_cast<unsigned*>(ws + L.header); a.nblocks = L.nblocks;
    a.partial = reinterpret_cast<double*>(ws + L.partial);
    a.n = n; a.sum_d = sum_d; a.hist = reinterpret_cast<unsigned long long*>(hist);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a.sel.total + AS_WAVES - 1) / AS_WAVES), block(AS_WAVES * 64);
    fo_for_width(F, [&](auto nt) { hipLaunchKernelGGL(as_fit_rows_kernel<decltype(nt)::value>, grid, block, 0, st, a); });
    hipLaunchKernelGGL(fo_count_kernel<AsArgs>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_base_kernel<AsArgs>, dim3(1), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_write_index_kernel<AsArgs>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    fo_for_width(F, [&](auto nt) { hipLaunchKernelGGL(as_fit_sum_kernel<decltype(nt)::value>, dim3(AS_CHUNKS), block, 0, st, a); });
    hipLaunchKernelGGL(as_fit_reduce_kernel, dim3(1), dim3(256), 0, st, a);
    return effdet_check_launch();
}
