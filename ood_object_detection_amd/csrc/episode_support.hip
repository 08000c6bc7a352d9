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
// over the rows whose nearest prototype it is, ascending rows, no atomics (pl_part_kernel of episode_rows.h); (3) one workgroup: bar P_k / bar Pdot_k complete, bar cmean /
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
    RowsSplit rows;
    PartsSplit parts, parts2;                         // of the first and the second pass
    PlKept kept;                                      // from the forward
    long long o_scratch, total;                       // in floats
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
SlPlan sl_plan(int n, int d, int m) {
    SlPlan p;
    p.rows = rows_split(n, PL_MAX_G);
    p.parts = parts_split(n, PL_MAX_PARTS);
    p.parts2 = parts_split(n, SL_MAX_PARTS2);
    long long o = pl_kept(n, d, m, p.kept);
    o += o & 1;                                       // float64 alignment of the scratch
    p.o_scratch = o;
    p.s1 = sl_scratch(n, d, m, p.rows.G, p.parts.parts, false);
    p.s2 = sl_scratch(n, d, m, p.rows.G, p.parts2.parts, true);
    const long long a = p.s1.total, b = 2 * p.s2.total;
    p.total = o + (a > b ? a : b);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------

// one workgroup: the prototype stage (P, cmean, pmean, tc, nv)
__global__ __launch_bounds__(1024) void sl_proto_kernel(const float* X, int n, int d, int m, const long long* proto0, const unsigned char* valid,
                                                        const long long* proto, float* P, float* cmean, float* pmean, float* tc,
                                                        float* nv_out) {
    __shared__ PlProtoLds L;
    pl_proto_stage(L, X, n, d, m, proto0, valid, proto, P, cmean, pmean, tc, nv_out);
}

// a wave per row
__global__ __launch_bounds__(256) void sl_fwd_rows_kernel(const float* X, const float* confs, const float* logits, int n, int d, int m,
                                                          int rows_per_block, float dot_mult, float dot_add, const float* dots,
                                                          const long long* nearest, int use_max, const float* P, const float* pmean,
                                                          const float* tc, float* inv, float* s, float* sim, float* target, float* fpart) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PlDots dt = pl_dots(dots, dot_mult, dot_add);
    int r1;
    const int r0 = pl_row_range(rows_per_block, n, r1);
    float sum = 0.f;
    for (int i = r0 + wave; i < r1; i += 4) {
        float v[PL_MAX_DL];
        const float iv = pl_load_row(X + (long long)i * d, d, lane, v);
        const float si = pl_sigmoid(dt.m * (confs[i] + dt.a));
        float T = 1.f;
        const float* prow = pl_proto_row(pl_nearest(nearest, i, m, use_max), d, P, pmean, tc, T);
        const float dot = pl_row_dot(v, iv, prow, d, lane);
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
            const double iv = 1.0 / fmax(sqrt(pl_wave_sum(ss)), 1e-12);
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) { e[q] *= iv; a += e[q] * w[q]; }
            a = pl_wave_sum(a);
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
        dot = pl_wave_sum(dot); dotd = pl_wave_sum(dotd);
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
    const PlDots dt = pl_dots(dots, dot_mult, dot_add);
    const R dm = dt.m, da = dt.a;
    const R g = gup[0], nf = (R)n;
    R Vm = 0, Va = 0;
    if (SECOND) { Vm = V.mult ? V.mult[0] : 0.f; Va = V.add ? V.add[0] : 0.f; }
    int r1;
    const int r0 = pl_row_range(rows_per_block, n, r1);
    R pm = 0, pa = 0, pl = 0;
    for (int i = r0 + wave; i < r1; i += 4) {
        const float* row = X + (long long)i * d;
        const R cf = confs[i], x = logits[i], l = dm * (cf + da);
        const float* vrow = (SECOND && V.e) ? V.e + (long long)i * d : nullptr;
        const int k = pl_nearest(nearest, i, m, use_max);
        R T = 1, Td = 0;
        const R* prow = pl_proto_row(k, d, P, pmean, tc, T);
        const R* pdrow = SECOND ? pl_proto_row(k, d, Pdot, pmd, tcd, Td) : pmd;
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
            iv = (R)1 / fmax(sqrt(pl_wave_sum(ss)), (R)1e-12);
            simi = 0;
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) {
                const int c = lane + 64 * q;
                e[q] *= iv;
                a += e[q] * w[q];
                if (c < d) { simi += e[q] * prow[c]; prw += prow[c] * w[q]; epd += e[q] * pdrow[c]; }
            }
            simi = pl_wave_sum(simi); a = pl_wave_sum(a); prw = pl_wave_sum(prw); epd = pl_wave_sum(epd);
            si = pl_sigmoid(l);
        } else {
            iv = inv[i]; si = s[i]; simi = sim[i];
#pragma unroll
            for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; e[q] = c < d ? row[c] * iv : (R)0; }
        }
        // s (1 - s) as sigmoid(l) sigmoid(-l): 1 - s is 0 in float32 from l = 17 on, the product is not
        const R t = (si * T) * simi, sx = pl_sigmoid(x), sp = si * pl_sigmoid(-l);
        R bt, btd = 0, dx, simdot = 0, ldot = 0, sdot = 0, vc = 0;
        if (SECOND) {
            simdot = (prw - simi * a) * iv + epd;                    // edot_i . P + e_i . Pdot
            vc = V.c ? V.c[i] : 0.f;
            if (thresh_grad) { ldot = Vm * (cf + da) + dm * (vc + Va); sdot = sp * ldot; }
            const R tdot = (sdot * T) * simi + (si * Td) * simi + (si * T) * simdot;
            const R vx = V.x ? V.x[i] : 0.f;
            pl += (sx - t) * vx - x * tdot;
            dx = g * ((sx * pl_sigmoid(-x)) * vx - tdot) / nf;
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
            iv = (R)1 / fmax(sqrt(pl_wave_sum(ss)), (R)1e-12);
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
        a = pl_wave_sum(a); u = pl_wave_sum(u); w = pl_wave_sum(w); eb = pl_wave_sum(eb);
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
        a = pl_wave_sum(a); b = pl_wave_sum(b); l = pl_wave_sum(l);
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
    const PlKept& k = p.kept;
    const PartsSplit& ps = SECOND ? p.parts2 : p.parts;
    R* x = reinterpret_cast<R*>(w + p.o_scratch);
    const R *P, *cmean, *pmean, *tc, *nv;
    if constexpr (SECOND) {
        hipLaunchKernelGGL(sl_tangent_kernel, dim3(1), dim3(1024), 0, st, embds, V.e, n, d, m, proto0, valid, proto, x + s.o_P, x + s.o_cmean,
                           x + s.o_pmean, x + s.o_tc, x + s.o_nv, x + s.o_Pdot, x + s.o_cmd, x + s.o_pmd, x + s.o_tcd);
        P = x + s.o_P; cmean = x + s.o_cmean; pmean = x + s.o_pmean; tc = x + s.o_tc; nv = x + s.o_nv;
    } else {
        P = w + k.o_P; cmean = w + k.o_cmean; pmean = w + k.o_pmean; tc = w + k.o_tc; nv = w + k.o_nv;
    }
    hipLaunchKernelGGL((sl_rows_kernel<SECOND, R>), dim3(p.rows.G), dim3(256), 0, st, embds, confs, logits, n, d, m, p.rows.rows_per_block,
                       dot_mult, dot_add, dots, nearest, use_max, thresh_grad, gup, V, P, pmean, tc, w + k.o_inv, w + k.o_s, w + k.o_sim,
                       x + s.o_Pdot, x + s.o_pmd, x + s.o_tcd, d_embds, d_confs, d_logits, x + s.o_rowc, x + s.o_fpart);
    hipLaunchKernelGGL((pl_part_kernel<SECOND, R>), dim3(ps.parts, use_max ? m : 1), dim3(256), 0, st, embds, V.e, nearest, n, d, m, ps.per, use_max,
                       x + s.o_rowc, x + s.o_BPpart, x + s.o_BPdpart, x + s.o_bTpart);
    hipLaunchKernelGGL((sl_bwd_proto_kernel<SECOND, R>), dim3(1), dim3(1024), 0, st, embds, V.e, n, d, m, ps.parts, p.rows.G, proto0, valid, proto,
                       use_max, P, cmean, nv, w + k.o_inv, x + s.o_Pdot, x + s.o_cmd, x + s.o_BPpart, x + s.o_BPdpart, x + s.o_bTpart,
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
    const PlKept& k = p.kept;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* w = workspace;
    float* fpart = w + p.o_scratch + p.s1.o_fpart;
    hipLaunchKernelGGL(sl_proto_kernel, dim3(1), dim3(1024), 0, st, embds, n, d, m, proto0, valid, proto, w + k.o_P, w + k.o_cmean, w + k.o_pmean,
                       w + k.o_tc, w + k.o_nv);
    hipLaunchKernelGGL(sl_fwd_rows_kernel, dim3(p.rows.G), dim3(256), 0, st, embds, confs, logits, n, d, m, p.rows.rows_per_block, dot_mult, dot_add,
                       dots, nearest, use_max, w + k.o_P, w + k.o_pmean, w + k.o_tc, w + k.o_inv, w + k.o_s, w + k.o_sim, target, fpart);
    hipLaunchKernelGGL(sl_final_kernel, dim3(1), dim3(64), 0, st, fpart, p.rows.G, n, loss);
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
