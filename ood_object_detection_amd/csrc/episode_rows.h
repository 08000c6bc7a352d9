// The shared layer of the three episode units (episode.hip, episode_loss.hip, episode_support.hip): the limits, the two splits of
// the rows, what a loss forward keeps for its backward, the row prologue of the wave-per-row kernels, the prototype stage and the
// part kernel.  All three units are built with -ffp-contract=off, so one text gives the same bits wherever it is used.
#pragma once
#include "common.h"

namespace {

constexpr int PL_MAX_DL = 8;              // d <= 64 * PL_MAX_DL
constexpr int PL_MAX_M = 64;
constexpr int PL_MAX_G = 1024;
constexpr int PL_MAX_PARTS = 32;

inline bool pl_shape_ok(int n, int d, int m) {
    return n > 0 && d > 0 && m > 0 && m <= PL_MAX_M && d <= 64 * PL_MAX_DL && (long long)m * d <= 16384 && n >= m;
}

// the rows in G blocks of rows_per_block (a wave per row, 16 rows a block unless that exceeds max_G blocks)
struct RowsSplit { int G, rows_per_block; };
inline RowsSplit rows_split(int n, int max_G) {
    RowsSplit r;
    r.G = (n + 15) / 16; if (r.G > max_G) r.G = max_G;
    r.rows_per_block = (n + r.G - 1) / r.G;
    r.G = (n + r.rows_per_block - 1) / r.rows_per_block;
    return r;
}
// the rows in `parts` runs of `per` (256 rows a part unless that exceeds max_parts)
struct PartsSplit { int parts, per; };
inline PartsSplit parts_split(int n, int max_parts) {
    PartsSplit p;
    p.parts = (n + 255) / 256; if (p.parts > max_parts) p.parts = max_parts;
    p.per = (n + p.parts - 1) / p.parts;
    p.parts = (n + p.per - 1) / p.per;
    return p;
}

// what a loss forward keeps in its workspace for the backward, from offset 0; returns the floats it takes
struct PlKept { long long o_inv, o_s, o_sim, o_tc, o_cmean, o_pmean, o_P, o_nv; };
inline long long pl_kept(int n, int d, int m, PlKept& k) {
    long long o = 0;
    k.o_inv = o; o += n;
    k.o_s = o; o += n;
    k.o_sim = o; o += n;
    k.o_tc = o; o += PL_MAX_M;
    k.o_cmean = o; o += d;
    k.o_pmean = o; o += d;
    k.o_P = o; o += (long long)m * d;
    k.o_nv = o; o += 1;
    return o;
}

DEV long long pl_clamp(long long v, long long hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

template <class R> DEV R pl_wave_sum(R v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- the row prologue of the wave-per-row kernels --------------------------------------------------------------------------

// dot_mult / dot_add: on the device when `dots` is given, else by value
struct PlDots { float m, a; };
DEV PlDots pl_dots(const float* dots, float dot_mult, float dot_add) {
    PlDots r;
    r.m = dots ? dots[0] : dot_mult; r.a = dots ? dots[1] : dot_add;
    return r;
}

// the block's rows [returned, r1)
DEV int pl_row_range(int rows_per_block, int n, int& r1) {
    const int r0 = blockIdx.x * rows_per_block;
    r1 = r0 + rows_per_block; if (r1 > n) r1 = n;
    return r0;
}

// the row in the lanes' registers (column lane + 64 k), returns 1 / max(||row||, 1e-12); columns past d add +0: the sum
// novelty_score_kernel forms
DEV float pl_load_row(const float* row, int d, int lane, float (&v)[PL_MAX_DL]) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) { const int c = lane + 64 * k; v[k] = c < d ? row[c] : 0.f; }
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) ss += v[k] * v[k];
    ss = wave_reduce_sum(ss);
    return 1.0f / fmaxf(sqrtf(ss), 1e-12f);
}

DEV float pl_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
DEV double pl_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

// the prototype row i is compared with: its nearest one ('max', clamped into [0, m)) or -1, the mean of all ('avg')
DEV int pl_nearest(const long long* nearest, int i, int m, int use_max) { return use_max ? (int)pl_clamp(nearest[i], m) : -1; }
// ... and that row of P with its entry of tc (k >= 0), or pmean, where T stays what the caller set
template <class R> DEV const R* pl_proto_row(int k, int d, const R* P, const R* pmean, const R* tc, R& T) {
    if (k < 0) return pmean;
    T = tc[k];
    return P + (long long)k * d;
}

// e_i . prow from the loaded row
DEV float pl_row_dot(const float (&v)[PL_MAX_DL], float iv, const float* prow, int d, int lane) {
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; if (c < d) dot += (v[q] * iv) * prow[c]; }
    return wave_reduce_sum(dot);
}

// ---- the prototype stage of a loss forward ---------------------------------------------------------------------------------

struct PlProtoLds {
    float vec[64 * PL_MAX_DL];
    float tc[PL_MAX_M], iv0[PL_MAX_M];
    long long r0[PL_MAX_M];
    int val[PL_MAX_M];
};

// one workgroup of 1024: P [m][d], cmean [d], pmean [d] = mean_k P_k, tc [m] (also left in L.tc, visible after the caller's
// __syncthreads), nv
DEV void pl_proto_stage(PlProtoLds& L, const float* X, int n, int d, int m, const long long* proto0, const unsigned char* valid,
                        const long long* proto, float* P, float* cmean, float* pmean, float* tc, float* nv_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = wave; k < m; k += 16) {
        float v[PL_MAX_DL];
        const long long r = pl_clamp(proto[k], n);
        const float iv = pl_load_row(X + r * d, d, lane, v);
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; if (c < d) P[(long long)k * d + c] = v[q] * iv; }
        const long long rr = pl_clamp(proto0[k], n);
        const float iv2 = pl_load_row(X + rr * d, d, lane, v);
        if (lane == 0) { L.iv0[k] = iv2; L.r0[k] = rr; L.val[k] = valid[k] ? 1 : 0; }
    }
    __syncthreads();
    int nv = 0;
    for (int k = 0; k < m; ++k) nv += L.val[k];
    const float nvf = (float)nv;
    for (int c = tid; c < d; c += 1024) {
        float t = 0.f, u = 0.f;
        for (int k = 0; k < m; ++k) {
            if (L.val[k]) t += X[L.r0[k] * d + c] * L.iv0[k];
            u += P[(long long)k * d + c];
        }
        const float cm = t / nvf;                                   // an empty valid set gives NaN, as the reference's mean does
        cmean[c] = cm; L.vec[c] = cm;
        pmean[c] = u / (float)m;
    }
    __syncthreads();
    for (int k = wave; k < m; k += 16) {
        float dot = 0.f;
        for (int c = lane; c < d; c += 64) dot += P[(long long)k * d + c] * L.vec[c];
        dot = wave_reduce_sum(dot);
        if (lane == 0) { tc[k] = dot; L.tc[k] = dot; }
    }
    if (tid == 0) nv_out[0] = nvf;
}

// ---- the part kernel of a loss backward ------------------------------------------------------------------------------------

// grid (part, prototype): over the part's rows with nearest == k, ascending rows per wave ('avg': one "prototype", every row),
// from the coefficients rowc[4 i ..] = (c1, c2, bT, bTd) the rows kernel left per row (R: float, or double in the support loss's
// second pass):  BPpart = sum c1_i r_i + c2_i V_e,i;  BPdpart = sum c2_i r_i;  bTpart = the sums of bT, bTd.  Slots 1 and 3 and
// BPdpart are read and written by SECOND only.
template <bool SECOND, class R>
__global__ __launch_bounds__(256) void pl_part_kernel(const float* X, const float* Ve, const long long* nearest, int n, int d, int m, int per,
                                                      int use_max, const R* rowc, R* BPpart, R* BPdpart, R* bTpart) {
    __shared__ R red[4][64 * PL_MAX_DL];
    __shared__ R redd[SECOND ? 4 : 1][64 * PL_MAX_DL];
    __shared__ R tcr[4][2];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.y, q = blockIdx.x, mm = gridDim.y;
    const int r0 = q * per;
    int r1 = r0 + per; if (r1 > n) r1 = n;
    R acc[PL_MAX_DL], accd[PL_MAX_DL];
#pragma unroll
    for (int u = 0; u < PL_MAX_DL; ++u) { acc[u] = 0; accd[u] = 0; }
    R ta = 0, tb = 0;
    for (int base = r0 + wave * 64; base < r1; base += 256) {
        const int i = base + lane;
        bool match = i < r1;
        if (match && use_max) match = (int)pl_clamp(nearest[i], m) == k;
        if (match) { ta += rowc[4LL * i + 2]; if (SECOND) tb += rowc[4LL * i + 3]; }
        unsigned long long mask = __ballot(match);
        while (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            const long long ii = base + b;
            const R c1 = rowc[4 * ii], c2 = SECOND ? rowc[4 * ii + 1] : (R)0;
            const float* row = X + ii * d;
            const float* vrow = (SECOND && Ve) ? Ve + ii * d : nullptr;
#pragma unroll
            for (int u = 0; u < PL_MAX_DL; ++u) {
                const int c = lane + 64 * u;
                if (c < d) {
                    const R r = row[c];
                    acc[u] += c1 * r;
                    if (SECOND) { if (vrow) acc[u] += c2 * (R)vrow[c]; accd[u] += c2 * r; }
                }
            }
        }
    }
    ta = pl_wave_sum(ta); tb = pl_wave_sum(tb);
#pragma unroll
    for (int u = 0; u < PL_MAX_DL; ++u) { red[wave][lane + 64 * u] = acc[u]; if (SECOND) redd[wave][lane + 64 * u] = accd[u]; }
    if (lane == 0) { tcr[wave][0] = ta; tcr[wave][1] = tb; }
    __syncthreads();
    const long long o = (long long)q * mm + k;
    for (int c = threadIdx.x; c < d; c += 256) {
        BPpart[o * d + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        if (SECOND) BPdpart[o * d + c] = ((redd[0][c] + redd[1][c]) + redd[2][c]) + redd[3][c];
    }
    if (threadIdx.x < 2) bTpart[2 * o + threadIdx.x] = ((tcr[0][threadIdx.x] + tcr[1][threadIdx.x]) + tcr[2][threadIdx.x]) + tcr[3][threadIdx.x];
}

}  // namespace
