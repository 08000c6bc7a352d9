// The meta phase's support loss (infer.py:645-658) on the decisions effdet_episode_cluster took: forward, backward and the backward
// of that backward, without any n x n matrix.  Symbols as in episode_loss.hip, x the class logits:
//     e_i = r_i inv_i, l_i = dot_mult (conf_i + dot_add), s_i = sigmoid(l_i), P_k = e[proto_k], cmean = mean of the valid e[proto0_v]
//     tc_k = P_k . cmean;  'max': sim_i = e_i . P[nearest_i], T_i = tc[nearest_i];  'avg': sim_i = e_i . mean_k P_k, T_i = 1
//     t_i = s_i T_i sim_i;  loss = (1/n) sum_i max(x_i, 0) - x_i t_i + log1p(exp(-|x_i|))
//
// Forward, three launches: one workgroup (P, cmean, mean_k P_k, tc), a wave per row (inv, s, sim kept; t; per-block partials of the
// sum), one wave that adds the partials in order.
//
// Backward and second backward are ONE chain, the reverse pass of a scalar through t and - in the second pass - through t's
// forward-mode tangent tdot along the cotangents V = (V_e, V_c, V_mult, V_add):
//     first:   the scalar is g loss:                          bar t_i = -g x_i / n,    bar tdot_i = 0,          d x_i = g (sigmoid(x_i) - t_i) / n
//     second:  the scalar is g Ldot, Ldot = (1/n) sum_i (sigmoid(x_i) - t_i) V_x,i - x_i tdot_i:
//                                                             bar t_i = -g V_x,i / n,  bar tdot_i = -g x_i / n, d x_i = g (sigmoid'(x_i) V_x,i - tdot_i) / n
// with the tangents  edot_i = (V_e,i - e_i a_i) inv_i, a_i = e_i . V_e,i;  ldot_i = V_mult (conf_i + dot_add) + dot_mult (V_c,i + V_add),
// sdot_i = s_i (1 - s_i) ldot_i;  Pdot_k = edot[proto_k], cmeandot, tcdot_k = Pdot_k . cmean + P_k . cmeandot;
// simdot_i = edot_i . P + e_i . Pdot;  tdot_i = sdot T sim + s Tdot sim + s T simdot.  The reverse pass then is, per row,
//     bar s = bar t T sim + bar tdot (Tdot sim + T simdot)        bar sdot   = bar tdot T sim
//     bar T = bar t s sim + bar tdot (sdot sim + s simdot)        bar Tdot   = bar tdot s sim
//     bar sim = bar t s T + bar tdot (sdot T + s Tdot)            bar simdot = bar tdot s T
//     bar l = (bar s + bar sdot ldot (1 - 2 s)) s (1 - s),  bar ldot = bar sdot s (1 - s)   (thresh_grad; else s is a constant)
//     bar e_i = bar sim P + bar simdot Pdot,  bar edot_i = bar simdot P;   bar P += bar sim e_i + bar simdot edot_i,  bar Pdot += bar simdot e_i
// and through the normalisation, for any row with (bar e, bar edot), u = bar edot . e, w = bar edot . V_e:
//     b = bar e - inv (u V_e + a bar edot),   bar r = inv (b - e (e . b)) - inv^2 (w - a u) e
// Three launches, as the projection-loss backward: (1) a wave per row: the row's own bar r, d conf, d x, per-block partials of
// d dot_mult / d dot_add / Ldot, and four per-row coefficients; (2) grid (part, prototype): [parts][m][d] partials of bar P and bar Pdot
// over the rows whose nearest prototype it is, ascending rows, no atomics; (3) one workgroup: bar P_k / bar Pdot_k complete, bar cmean /
// bar cmeandot, through the normalisation into the rows proto_k / proto0_k one after the other, and the scalar sums.  The second pass
// runs one more launch first: one workgroup forms Pdot, cmeandot, mean_k Pdot_k and tcdot.  A null cotangent is zero.
// Forward and backward compute in float32.  The second pass computes in float64 from the float32 inputs (its own P, cmean, tc, inv,
// s, sim; partials in float64 over at most 16 parts) and rounds once on the way out: its scalar results (d g, d dot_mult, d dot_add)
// are sums of n terms of both signs, and a float32 chain leaves them with an error of several ulp of the TERMS, which is what the outer
// gradient of the meta phase is made of.  The scratch of the two passes shares one region of the workspace.
// Every reduction has a fixed order: two calls give the same bits.  proto / proto0 are clamped into [0, n) and nearest into [0, m).
#include <cstdint>

#include "episode_rows.h"

namespace {

constexpr int SL_MAX_PARTS2 = 16;         // the second pass keeps its partials in float64: half as many parts, the same bytes

struct SlScratch {                        // a pass's scratch, in units of its own number type
    long long o_fpart, o_rowc, o_BPpart, o_BPdpart, o_bTpart, o_BP, o_BPd, o_P, o_cmean, o_pmean, o_tc, o_nv, o_Pdot, o_cmd, o_pmd, o_tcd, total;
};
struct SlPlan {
    int G, rows_per_block, parts, per, parts2, per2;
    long long o_inv, o_s, o_sim, o_tc, o_cmean, o_pmean, o_P, o_nv, o_scratch, total;       // kept from the forward; scratch, in floats
    SlScratch s1, s2;
};
SlScratch sl_scratch(int n, int d, int m, int G, int parts, bool second) {
    const long long md = (long long)m * d;
    SlScratch s;
    long long o = 0;
    s.o_fpart = o; o += 4LL * G;
    s.o_rowc = o; o += 4LL * n;
    s.o_BPpart = o; o += parts * md;
    s.o_BPdpart = o; o += second ? parts * md : 0;
    s.o_bTpart = o; o += 2LL * parts * m;
    s.o_BP = o; o += md;
    s.o_BPd = o; o += second ? md : 0;
    s.o_P = o; o += second ? md : 0;                  // the second pass forms its own float64 P, cmean, pmean, tc, nv
    s.o_cmean = o; o += second ? d : 0;
    s.o_pmean = o; o += second ? d : 0;
    s.o_tc = o; o += second ? PL_MAX_M : 0;
    s.o_nv = o; o += second ? 1 : 0;
    s.o_Pdot = o; o += second ? md : 0;
    s.o_cmd = o; o += second ? d : 0;
    s.o_pmd = o; o += second ? d : 0;
    s.o_tcd = o; o += second ? PL_MAX_M : 0;
    s.total = o;
    return s;
}
void sl_split(int n, int max_parts, int& parts, int& per) {
    parts = (n + 255) / 256; if (parts > max_parts) parts = max_parts;
    per = (n + parts - 1) / parts;
    parts = (n + per - 1) / per;
}
SlPlan sl_plan(int n, int d, int m) {
    SlPlan p;
    p.G = (n + 15) / 16; if (p.G > PL_MAX_G) p.G = PL_MAX_G;
    p.rows_per_block = (n + p.G - 1) / p.G;
    p.G = (n + p.rows_per_block - 1) / p.rows_per_block;
    sl_split(n, PL_MAX_PARTS, p.parts, p.per);
    sl_split(n, SL_MAX_PARTS2, p.parts2, p.per2);
    long long o = 0;
    p.o_inv = o; o += n;
    p.o_s = o; o += n;
    p.o_sim = o; o += n;
    p.o_tc = o; o += PL_MAX_M;
    p.o_cmean = o; o += d;
    p.o_pmean = o; o += d;
    p.o_P = o; o += (long long)m * d;
    p.o_nv = o; o += 1;
    o += o & 1;                                       // float64 alignment of the scratch
    p.o_scratch = o;
    p.s1 = sl_scratch(n, d, m, p.G, p.parts, false);
    p.s2 = sl_scratch(n, d, m, p.G, p.parts2, true);
    const long long a = p.s1.total, b = 2 * p.s2.total;
    p.total = o + (a > b ? a : b);
    return p;
}

DEV float sl_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
DEV double sl_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }
template <class R> DEV R sl_wave_sum(R v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------

// one workgroup: P [m][d], cmean [d], pmean [d] = mean_k P_k, tc [m], nv
__global__ __launch_bounds__(1024) void sl_proto_kernel(const float* X, int n, int d, int m, const long long* proto0, const unsigned char* valid,
                                                        const long long* proto, float* P, float* cmean, float* pmean, float* tc,
                                                        float* nv_out) {
    __shared__ float vec[64 * PL_MAX_DL];
    __shared__ float iv0[PL_MAX_M];
    __shared__ long long r0[PL_MAX_M];
    __shared__ int val[PL_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = wave; k < m; k += 16) {
        float v[PL_MAX_DL];
        const long long r = pl_clamp(proto[k], n);
        const float iv = pl_load_row(X + r * d, d, lane, v);
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; if (c < d) P[(long long)k * d + c] = v[q] * iv; }
        const long long rr = pl_clamp(proto0[k], n);
        const float iv2 = pl_load_row(X + rr * d, d, lane, v);
        if (lane == 0) { iv0[k] = iv2; r0[k] = rr; val[k] = valid[k] ? 1 : 0; }
    }
    __syncthreads();
    int nv = 0;
    for (int k = 0; k < m; ++k) nv += val[k];
    const float nvf = (float)nv;
    for (int c = tid; c < d; c += 1024) {
        float t = 0.f, u = 0.f;
        for (int k = 0; k < m; ++k) {
            if (val[k]) t += X[r0[k] * d + c] * iv0[k];
            u += P[(long long)k * d + c];
        }
        const float cm = t / nvf;                                   // an empty valid set gives NaN, as the reference's mean does
        cmean[c] = cm; vec[c] = cm;
        pmean[c] = u / (float)m;
    }
    __syncthreads();
    for (int k = wave; k < m; k += 16) {
        float dot = 0.f;
        for (int c = lane; c < d; c += 64) dot += P[(long long)k * d + c] * vec[c];
        dot = wave_reduce_sum(dot);
        if (lane == 0) tc[k] = dot;
    }
    if (tid == 0) nv_out[0] = nvf;
}

// a wave per row
__global__ __launch_bounds__(256) void sl_fwd_rows_kernel(const float* X, const float* confs, const float* logits, int n, int d, int m,
                                                          int rows_per_block, float dot_mult, float dot_add, const float* dots,
                                                          const long long* nearest, int use_max, const float* P, const float* pmean,
                                                          const float* tc, float* inv, float* s, float* sim, float* target, float* fpart) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float dm = dots ? dots[0] : dot_mult, da = dots ? dots[1] : dot_add;
    const int r0 = blockIdx.x * rows_per_block;
    int r1 = r0 + rows_per_block; if (r1 > n) r1 = n;
    float sum = 0.f;
    for (int i = r0 + wave; i < r1; i += 4) {
        float v[PL_MAX_DL];
        const float iv = pl_load_row(X + (long long)i * d, d, lane, v);
        const float si = sl_sigmoid(dm * (confs[i] + da));
        const float* prow = pmean;
        float T = 1.f;
        if (use_max) {
            const int k = (int)pl_clamp(nearest[i], m);
            prow = P + (long long)k * d; T = tc[k];
        }
        float dot = 0.f;
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; if (c < d) dot += (v[q] * iv) * prow[c]; }
        dot = wave_reduce_sum(dot);
        const float t = (si * T) * dot, x = logits[i];
        sum += (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
        if (lane == 0) { inv[i] = iv; s[i] = si; sim[i] = dot; target[i] = t; }
    }
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) fpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave: the G partials in a fixed order
__global__ __launch_bounds__(64) void sl_final_kernel(const float* fpart, int G, int n, float* loss) {
    float sum = 0.f;
    for (int b = threadIdx.x; b < G; b += 64) sum += fpart[b];
    sum = wave_reduce_sum(sum);
    if (threadIdx.x == 0) loss[0] = sum / (float)n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward (SECOND = false, float32 on what the forward kept) and the backward of the backward (SECOND = true, float64 inside)
// ---------------------------------------------------------------------------------------------------------------------------

// second pass, (0) one workgroup, float64: P, cmean, pmean, tc, nv again and their tangents Pdot [m][d], cmeandot [d], pmeandot [d], tcdot [m]
__global__ __launch_bounds__(1024) void sl_tangent_kernel(const float* X, const float* Ve, int n, int d, int m, const long long* proto0,
                                                          const unsigned char* valid, const long long* proto, double* P, double* cmean,
                                                          double* pmean, double* tc, double* nv_out, double* Pdot, double* cmd,
                                                          double* pmd, double* tcd) {
    __shared__ double vec[64 * PL_MAX_DL], vecd[64 * PL_MAX_DL];
    __shared__ double a0[PL_MAX_M], iv0[PL_MAX_M];
    __shared__ long long r0[PL_MAX_M];
    __shared__ int val[PL_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = wave; k < m; k += 16) {
        for (int pass = 0; pass < 2; ++pass) {
            const long long r = pl_clamp(pass ? proto0[k] : proto[k], n);
            double e[PL_MAX_DL], w[PL_MAX_DL], ss = 0., a = 0.;
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) {
                const int c = lane + 64 * q;
                e[q] = c < d ? (double)X[r * d + c] : 0.;
                w[q] = (Ve && c < d) ? (double)Ve[r * d + c] : 0.;
                ss += e[q] * e[q];
            }
            const double iv = 1.0 / fmax(sqrt(sl_wave_sum(ss)), 1e-12);
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) { e[q] *= iv; a += e[q] * w[q]; }
            a = sl_wave_sum(a);
            if (pass == 0) {
#pragma unroll
                for (int q = 0; q < PL_MAX_DL; ++q) {
                    const int c = lane + 64 * q;
                    if (c < d) { P[(long long)k * d + c] = e[q]; Pdot[(long long)k * d + c] = (w[q] - e[q] * a) * iv; }
                }
            } else if (lane == 0) { a0[k] = a; iv0[k] = iv; r0[k] = r; val[k] = valid[k] ? 1 : 0; }
        }
    }
    __syncthreads();
    int nv = 0;
    for (int k = 0; k < m; ++k) nv += val[k];
    const double nvf = (double)nv;
    for (int c = tid; c < d; c += 1024) {
        double t = 0., td = 0., u = 0., ud = 0.;
        for (int k = 0; k < m; ++k) {
            if (val[k]) {
                const long long r = r0[k];
                const double e = (double)X[r * d + c] * iv0[k];
                t += e;
                td += ((Ve ? (double)Ve[r * d + c] : 0.) - e * a0[k]) * iv0[k];
            }
            u += P[(long long)k * d + c];
            ud += Pdot[(long long)k * d + c];
        }
        cmean[c] = vec[c] = t / nvf;                                // an empty valid set gives NaN
        cmd[c] = vecd[c] = td / nvf;
        pmean[c] = u / (double)m;
        pmd[c] = ud / (double)m;
    }
    __syncthreads();
    for (int k = wave; k < m; k += 16) {
        double dot = 0., dotd = 0.;
        for (int c = lane; c < d; c += 64) {
            const double p = P[(long long)k * d + c];
            dot += p * vec[c];
            dotd += Pdot[(long long)k * d + c] * vec[c] + p * vecd[c];
        }
        dot = sl_wave_sum(dot); dotd = sl_wave_sum(dotd);
        if (lane == 0) { tc[k] = dot; tcd[k] = dotd; }
    }
    if (tid == 0) nv_out[0] = nvf;
}

struct SlV { const float *e, *c, *x, *mult, *add; };        // the cotangents of the second pass, null = zero

// (1) a wave per row.  R: float on the kept inv / s / sim (first pass), double on its own (second pass)
template <bool SECOND, class R>
__global__ __launch_bounds__(256) void sl_rows_kernel(const float* X, const float* confs, const float* logits, int n, int d, int m,
                                                      int rows_per_block, float dot_mult, float dot_add, const float* dots,
                                                      const long long* nearest, int use_max, int thresh_grad, const float* gup, SlV V,
                                                      const R* P, const R* pmean, const R* tc, const float* inv, const float* s,
                                                      const float* sim, const R* Pdot, const R* pmd, const R* tcd, float* dE,
                                                      float* dconf, float* dlogit, R* rowc, R* fpart) {
    __shared__ R red[4][3];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const R dm = dots ? dots[0] : dot_mult, da = dots ? dots[1] : dot_add;
    const R g = gup[0], nf = (R)n;
    R Vm = 0, Va = 0;
    if (SECOND) { Vm = V.mult ? V.mult[0] : 0.f; Va = V.add ? V.add[0] : 0.f; }
    const int r0 = blockIdx.x * rows_per_block;
    int r1 = r0 + rows_per_block; if (r1 > n) r1 = n;
    R pm = 0, pa = 0, pl = 0;
    for (int i = r0 + wave; i < r1; i += 4) {
        const float* row = X + (long long)i * d;
        const R cf = confs[i], x = logits[i], l = dm * (cf + da);
        const float* vrow = (SECOND && V.e) ? V.e + (long long)i * d : nullptr;
        const R* prow = pmean;
        const R* pdrow = pmd;
        R T = 1, Td = 0;
        if (use_max) {
            const int k = (int)pl_clamp(nearest[i], m);
            prow = P + (long long)k * d; T = tc[k];
            if (SECOND) { pdrow = Pdot + (long long)k * d; Td = tcd[k]; }
        }
        R e[PL_MAX_DL], w[PL_MAX_DL];
        R iv, si, simi, a = 0, prw = 0, epd = 0;
        if (SECOND) {
            R ss = 0;
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) {
                const int c = lane + 64 * q;
                e[q] = c < d ? (R)row[c] : (R)0;
                w[q] = (vrow && c < d) ? (R)vrow[c] : (R)0;
                ss += e[q] * e[q];
            }
            iv = (R)1 / fmax(sqrt(sl_wave_sum(ss)), (R)1e-12);
            simi = 0;
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) {
                const int c = lane + 64 * q;
                e[q] *= iv;
                a += e[q] * w[q];
                if (c < d) { simi += e[q] * prow[c]; prw += prow[c] * w[q]; epd += e[q] * pdrow[c]; }
            }
            simi = sl_wave_sum(simi); a = sl_wave_sum(a); prw = sl_wave_sum(prw); epd = sl_wave_sum(epd);
            si = sl_sigmoid(l);
        } else {
            iv = inv[i]; si = s[i]; simi = sim[i];
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; e[q] = c < d ? row[c] * iv : (R)0; }
        }
        // s (1 - s) as sigmoid(l) sigmoid(-l): 1 - s is 0 in float32 from l = 17 on, the product is not
        const R t = (si * T) * simi, sx = sl_sigmoid(x), sp = si * sl_sigmoid(-l);
        R bt, btd = 0, dx, simdot = 0, ldot = 0, sdot = 0, vc = 0;
        if (SECOND) {
            simdot = (prw - simi * a) * iv + epd;                    // edot_i . P + e_i . Pdot
            vc = V.c ? V.c[i] : 0.f;
            if (thresh_grad) { ldot = Vm * (cf + da) + dm * (vc + Va); sdot = sp * ldot; }
            const R tdot = (sdot * T) * simi + (si * Td) * simi + (si * T) * simdot;
            const R vx = V.x ? V.x[i] : 0.f;
            pl += (sx - t) * vx - x * tdot;
            dx = g * ((sx * sl_sigmoid(-x)) * vx - tdot) / nf;
            bt = -(g * vx) / nf; btd = -(g * x) / nf;
        } else {
            dx = g * (sx - t) / nf;
            bt = -(g * x) / nf;
        }
        R bs = (bt * T) * simi, bT = (bt * si) * simi, bsim = (bt * si) * T, bsdot = 0, bTd = 0, bsimd = 0;
        if (SECOND) {
            bs += btd * (Td * simi + T * simdot);
            bT += btd * (sdot * simi + si * simdot);
            bsim += btd * (sdot * T + si * Td);
            bsdot = (btd * T) * simi; bTd = (btd * si) * simi; bsimd = (btd * si) * T;
        }
        R dc = 0;
        if (thresh_grad) {
            const R bl = (bs + bsdot * ldot * ((R)1 - (R)2 * si)) * sp, bld = bsdot * sp;
            dc = bl * dm + bld * Vm;
            pm += bl * (cf + da) + bld * (vc + Va);
            pa += bl * dm + bld * Vm;
        }
        // through the normalisation: bar e = bsim P + bsimd Pdot, bar edot = bsimd P
        const R u = bsimd * simi, ww = bsimd * prw;
        const R eb = bsim * simi + bsimd * epd - iv * ((R)2 * u * a);
        const R tail = iv * (ww - a * u);
        float* out = dE + (long long)i * d;
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) {
            const int c = lane + 64 * q;
            if (c < d) {
                R b = bsim * prow[c];
                if (SECOND) b += bsimd * pdrow[c] - iv * (u * w[q] + a * (bsimd * prow[c]));
                out[c] = (float)((b - e[q] * eb - tail * e[q]) * iv);
            }
        }
        if (lane == 0) {
            dconf[i] = (float)dc; dlogit[i] = (float)dx;
            R* rc = rowc + 4LL * i;
            rc[0] = bsim * iv - (bsimd * a) * (iv * iv); rc[1] = bsimd * iv; rc[2] = use_max ? bT : (R)0; rc[3] = use_max ? bTd : (R)0;
        }
    }
    if (lane == 0) { red[wave][0] = pm; red[wave][1] = pa; red[wave][2] = pl; }
    __syncthreads();
    if (threadIdx.x < 3) fpart[(long long)blockIdx.x * 4 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// (2) grid (part, prototype): over the part's rows with nearest == k, ascending rows per wave ('avg': one "prototype", every row),
// BPpart = sum c1_i r_i + c2_i V_e,i;  BPdpart = sum c2_i r_i;  bTpart = sums of bar T, bar Tdot
template <bool SECOND, class R>
__global__ __launch_bounds__(256) void sl_part_kernel(const float* X, const float* Ve, const long long* nearest, int n, int d, int m, int per,
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
    ta = sl_wave_sum(ta); tb = sl_wave_sum(tb);
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

// (3) one workgroup: the prototype gradients, through the normalisation into dE's rows; d dot_mult, d dot_add, Ldot
template <bool SECOND, class R>
__global__ __launch_bounds__(1024) void sl_bwd_proto_kernel(const float* X, const float* Ve, int n, int d, int m, int parts, int G,
                                                            const long long* proto0, const unsigned char* valid, const long long* proto,
                                                            int use_max, const R* P, const R* cmean, const R* nv_in, const float* inv,
                                                            const R* Pdot, const R* cmd, const R* BPpart, const R* BPdpart,
                                                            const R* bTpart, const R* fpart, R* BP, R* BPd, float* dE, float* ddots,
                                                            float* dgrad) {
    __shared__ R bcm[64 * PL_MAX_DL], bcmd[64 * PL_MAX_DL];
    __shared__ R btc[PL_MAX_M], btcd[PL_MAX_M];
    __shared__ R riv[2][PL_MAX_M], ra[2][PL_MAX_M], ru[2][PL_MAX_M], rw[2][PL_MAX_M], reb[2][PL_MAX_M];   // [0]: row proto_k, [1]: row proto0_k
    __shared__ long long rr[2][PL_MAX_M];
    __shared__ int val[PL_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < m) {
        const int k = tid;
        R a = 0, b = 0;
        if (use_max)
            for (int q = 0; q < parts; ++q) { a += bTpart[2 * ((long long)q * m + k)]; if (SECOND) b += bTpart[2 * ((long long)q * m + k) + 1]; }
        btc[k] = a; btcd[k] = b;
        rr[0][k] = pl_clamp(proto[k], n); rr[1][k] = pl_clamp(proto0[k], n); val[k] = valid[k] ? 1 : 0;
    }
    __syncthreads();
    const int md = m * d;
    for (int idx = tid; idx < md; idx += 1024) {
        const int k = idx / d, c = idx - k * d;
        R t = 0, td = 0;
        if (use_max) {
            for (int q = 0; q < parts; ++q) {
                t += BPpart[((long long)q * m + k) * d + c];
                if (SECOND) td += BPdpart[((long long)q * m + k) * d + c];
            }
        } else {
            for (int q = 0; q < parts; ++q) {
                t += BPpart[(long long)q * d + c];
                if (SECOND) td += BPdpart[(long long)q * d + c];
            }
            t /= (R)m; td /= (R)m;
        }
        if (use_max) {                                               // 'avg' does not read cmean, which is NaN for an empty valid set
            t += btc[k] * cmean[c];
            if (SECOND) { t += btcd[k] * cmd[c]; td += btcd[k] * cmean[c]; }
        }
        if (SECOND) BPd[idx] = td;
        BP[idx] = t;
    }
    const R nvf = nv_in[0];
    for (int c = tid; c < d; c += 1024) {
        R t = 0, td = 0;
        if (use_max) {
            for (int k = 0; k < m; ++k) {
                t += btc[k] * P[(long long)k * d + c];
                if (SECOND) { t += btcd[k] * Pdot[(long long)k * d + c]; td += btcd[k] * P[(long long)k * d + c]; }
            }
            t /= nvf; td /= nvf;
        }
        bcm[c] = t; bcmd[c] = td;
    }
    __syncthreads();
    // per row: a = e . V_e, u = bar edot . e, w = bar edot . V_e, eb = e . (bar e - inv (u V_e + a bar edot)) = e . bar e - 2 inv u a
    for (int j = wave; j < 2 * m; j += 16) {
        const int which = j >= m, k = which ? j - m : j;
        const long long r = rr[which][k];
        R iv;
        if (SECOND) {
            R ss = 0;
            for (int c = lane; c < d; c += 64) { const R v = X[r * d + c]; ss += v * v; }
            iv = (R)1 / fmax(sqrt(sl_wave_sum(ss)), (R)1e-12);
        } else {
            iv = inv[r];
        }
        R a = 0, u = 0, w = 0, eb = 0;
        for (int c = lane; c < d; c += 64) {
            const R e = (R)X[r * d + c] * iv;
            const R be = which ? bcm[c] : BP[(long long)k * d + c];
            eb += e * be;
            if (SECOND) {
                const R v = Ve ? (R)Ve[r * d + c] : (R)0, bed = which ? bcmd[c] : BPd[(long long)k * d + c];
                a += e * v; u += bed * e; w += bed * v;
            }
        }
        a = sl_wave_sum(a); u = sl_wave_sum(u); w = sl_wave_sum(w); eb = sl_wave_sum(eb);
        if (lane == 0) { riv[which][k] = iv; ra[which][k] = a; ru[which][k] = u; rw[which][k] = w; reb[which][k] = eb - iv * ((R)2 * u * a); }
    }
    __syncthreads();
    for (int c = tid; c < d; c += 1024) {
        for (int j = 0; j < 2 * m; ++j) {
            const int which = j >= m, k = which ? j - m : j;
            if (which && (!val[k] || !use_max)) continue;
            const long long r = rr[which][k];
            const R iv = riv[which][k], e = (R)X[r * d + c] * iv;
            R b = which ? bcm[c] : BP[(long long)k * d + c];
            R tail = 0;
            if (SECOND) {
                const R v = Ve ? (R)Ve[r * d + c] : (R)0, bed = which ? bcmd[c] : BPd[(long long)k * d + c];
                b -= iv * (ru[which][k] * v + ra[which][k] * bed);
                tail = iv * (rw[which][k] - ra[which][k] * ru[which][k]);
            }
            dE[r * d + c] += (float)((b - e * reb[which][k] - tail * e) * iv);
        }
    }
    if (wave == 15) {
        R a = 0, b = 0, l = 0;
        for (int g = lane; g < G; g += 64) { a += fpart[4 * g]; b += fpart[4 * g + 1]; if (SECOND) l += fpart[4 * g + 2]; }
        a = sl_wave_sum(a); b = sl_wave_sum(b); l = sl_wave_sum(l);
        if (lane == 0) { ddots[0] = (float)a; ddots[1] = (float)b; if (SECOND) dgrad[0] = (float)(l / (R)n); }
    }
}

bool sl_args_ok(const void* embds, const void* confs, const void* logits, int n, int d, int m, const void* proto0, const void* valid,
                const void* proto, const void* nearest, int use_max, const void* workspace, long long workspace_floats) {
    if (!embds || !confs || !logits || !proto0 || !valid || !proto || !workspace || !pl_shape_ok(n, d, m)) return false;
    if (use_max && !nearest) return false;
    return workspace_floats >= sl_plan(n, d, m).total;
}

template <bool SECOND, class R>
int sl_backward(hipStream_t st, const float* embds, const float* confs, const float* logits, int n, int d, int m, float dot_mult,
                float dot_add, const float* dots, const long long* proto0, const unsigned char* valid, const long long* proto,
                const long long* nearest, int use_max, int thresh_grad, const float* gup, SlV V, float* w, float* d_grad, float* d_embds,
                float* d_confs, float* d_logits, float* d_dots) {
    const SlPlan p = sl_plan(n, d, m);
    const SlScratch& s = SECOND ? p.s2 : p.s1;
    const int parts = SECOND ? p.parts2 : p.parts, per = SECOND ? p.per2 : p.per;
    R* x = reinterpret_cast<R*>(w + p.o_scratch);
    const R *P, *cmean, *pmean, *tc, *nv;
    if constexpr (SECOND) {
        hipLaunchKernelGGL(sl_tangent_kernel, dim3(1), dim3(1024), 0, st, embds, V.e, n, d, m, proto0, valid, proto, x + s.o_P, x + s.o_cmean,
                           x + s.o_pmean, x + s.o_tc, x + s.o_nv, x + s.o_Pdot, x + s.o_cmd, x + s.o_pmd, x + s.o_tcd);
        P = x + s.o_P; cmean = x + s.o_cmean; pmean = x + s.o_pmean; tc = x + s.o_tc; nv = x + s.o_nv;
    } else {
        P = w + p.o_P; cmean = w + p.o_cmean; pmean = w + p.o_pmean; tc = w + p.o_tc; nv = w + p.o_nv;
    }
    hipLaunchKernelGGL((sl_rows_kernel<SECOND, R>), dim3(p.G), dim3(256), 0, st, embds, confs, logits, n, d, m, p.rows_per_block, dot_mult,
                       dot_add, dots, nearest, use_max, thresh_grad, gup, V, P, pmean, tc, w + p.o_inv, w + p.o_s, w + p.o_sim,
                       x + s.o_Pdot, x + s.o_pmd, x + s.o_tcd, d_embds, d_confs, d_logits, x + s.o_rowc, x + s.o_fpart);
    hipLaunchKernelGGL((sl_part_kernel<SECOND, R>), dim3(parts, use_max ? m : 1), dim3(256), 0, st, embds, V.e, nearest, n, d, m, per, use_max,
                       x + s.o_rowc, x + s.o_BPpart, x + s.o_BPdpart, x + s.o_bTpart);
    hipLaunchKernelGGL((sl_bwd_proto_kernel<SECOND, R>), dim3(1), dim3(1024), 0, st, embds, V.e, n, d, m, parts, p.G, proto0, valid, proto,
                       use_max, P, cmean, nv, w + p.o_inv, x + s.o_Pdot, x + s.o_cmd, x + s.o_BPpart, x + s.o_BPdpart, x + s.o_bTpart,
                       x + s.o_fpart, x + s.o_BP, x + s.o_BPd, d_embds, d_dots, d_grad);
    return effdet_check_launch();
}

}  // namespace

extern "C" long long effdet_episode_supp_loss_workspace_floats(int n, int d, int m) {
    if (!pl_shape_ok(n, d, m)) return -1;
    return sl_plan(n, d, m).total;
}

extern "C" int effdet_episode_supp_loss(void* stream, const float* embds, const float* confs, const float* logits, int n, int d, int m,
                                        float dot_mult, float dot_add, const float* dots, const long long* proto0,
                                        const unsigned char* valid, const long long* proto, const long long* nearest, int use_max,
                                        float* workspace, long long workspace_floats, float* loss, float* target) {
    EFFDET_ENTER();
    if (!loss || !target || !sl_args_ok(embds, confs, logits, n, d, m, proto0, valid, proto, nearest, use_max, workspace, workspace_floats))
        return EFFDET_EINVAL;
    const SlPlan p = sl_plan(n, d, m);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* w = workspace;
    hipLaunchKernelGGL(sl_proto_kernel, dim3(1), dim3(1024), 0, st, embds, n, d, m, proto0, valid, proto, w + p.o_P, w + p.o_cmean, w + p.o_pmean,
                       w + p.o_tc, w + p.o_nv);
    hipLaunchKernelGGL(sl_fwd_rows_kernel, dim3(p.G), dim3(256), 0, st, embds, confs, logits, n, d, m, p.rows_per_block, dot_mult, dot_add, dots,
                       nearest, use_max, w + p.o_P, w + p.o_pmean, w + p.o_tc, w + p.o_inv, w + p.o_s, w + p.o_sim, target, w + p.o_scratch + p.s1.o_fpart);
    hipLaunchKernelGGL(sl_final_kernel, dim3(1), dim3(64), 0, st, w + p.o_scratch + p.s1.o_fpart, p.G, n, loss);
    return effdet_check_launch();
}

extern "C" int effdet_episode_supp_loss_backward(void* stream, const float* embds, const float* confs, const float* logits, int n, int d,
                                                 int m, float dot_mult, float dot_add, const float* dots, const long long* proto0,
                                                 const unsigned char* valid, const long long* proto, const long long* nearest,
                                                 int use_max, int thresh_grad, const float* grad_loss, float* workspace,
                                                 long long workspace_floats, float* d_embds, float* d_confs, float* d_logits,
                                                 float* d_dots) {
    EFFDET_ENTER();
    if (!grad_loss || !d_embds || !d_confs || !d_logits || !d_dots ||
        !sl_args_ok(embds, confs, logits, n, d, m, proto0, valid, proto, nearest, use_max, workspace, workspace_floats))
        return EFFDET_EINVAL;
    return sl_backward<false, float>(reinterpret_cast<hipStream_t>(stream), embds, confs, logits, n, d, m, dot_mult, dot_add, dots, proto0, valid,
                              proto, nearest, use_max, thresh_grad, grad_loss, SlV{nullptr, nullptr, nullptr, nullptr, nullptr}, workspace,
                              nullptr, d_embds, d_confs, d_logits, d_dots);
}

extern "C" int effdet_episode_supp_loss_backward2(void* stream, const float* embds, const float* confs, const float* logits, int n, int d,
                                                  int m, float dot_mult, float dot_add, const float* dots, const long long* proto0,
                                                  const unsigned char* valid, const long long* proto, const long long* nearest,
                                                  int use_max, int thresh_grad, const float* grad_loss, const float* v_embds,
                                                  const float* v_confs, const float* v_logits, const float* v_mult, const float* v_add,
                                                  float* workspace, long long workspace_floats, float* d_grad, float* h_embds,
                                                  float* h_confs, float* h_logits, float* h_dots) {
    EFFDET_ENTER();
    if (!grad_loss || !d_grad || !h_embds || !h_confs || !h_logits || !h_dots || (reinterpret_cast<uintptr_t>(workspace) & 7) ||
        !sl_args_ok(embds, confs, logits, n, d, m, proto0, valid, proto, nearest, use_max, workspace, workspace_floats))
        return EFFDET_EINVAL;
    return sl_backward<true, double>(reinterpret_cast<hipStream_t>(stream), embds, confs, logits, n, d, m, dot_mult, dot_add, dots, proto0, valid,
                             proto, nearest, use_max, thresh_grad, grad_loss, SlV{v_embds, v_confs, v_logits, v_mult, v_add}, workspace,
                             d_grad, h_embds, h_confs, h_logits, h_dots);
}
