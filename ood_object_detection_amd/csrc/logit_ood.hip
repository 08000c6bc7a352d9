// Logit-space OOD scores on the device: maximum softmax probability, softmax entropy, generalized entropy (GEN, Liu et al. 2023),
// JointEnergy (Wang et al. 2021), KL matching against class templates (Hendrycks et al. 2022) and the standardized max logit
// (Jung et al. 2021), all from one read of a row of C class logits.
//
//   per row, float32, z the C logits (bfloat16 widened exactly), u = z / T:
//     m = max u, k* = the lowest argmax;  e_k = exp(u_k - m), s = sum e, lse = m + log s, l_k = u_k - lse, p_k = exp(l_k)
//     msp = exp(m - lse);  neg_entropy = sum p_k l_k
//     gen = -sum over the top_m largest u_k (equal values: the lower k first) of exp(gamma * (l_k + q_k)),
//           q_k = log1p(-p_k) for k != k*, q_k* = log(sum_{k != k*} e_k) - log s
//     joint_energy = sum max(z_k, 0) + log1p(exp(-|z_k|))
//     with p, neg_entropy taken at T = 1:  kl_c = (neg_entropy - sum_k p_k logD_ck) + kl_inf_c,  kl_matching = -min_c kl_c
//     standardized = (max z - mu_k*) * inv_sigma_k*
//
//   score   16 rows per workgroup of four waves.  A wave takes four rows one after the other: lane t holds classes t, t + 64, ...
//           in registers, every sum runs over a lane's classes ascending and then over the lanes by the xor tree 32 .. 1, the
//           top_m cut is a 32-step search on the ordered bit pattern of u with ballots, so nothing leaves the wave.  p (T = 1) is
//           staged in LDS - zero beyond C and in rows that do not count - and the 16 x Cp by Cp x Cp product with log D runs on
//           the float32-input MFMA (16x16x4), wave w taking the class tiles w, w + 4, ...; beyond 512 classes p passes through
//           LDS in two K-chunks of 512, the second one recomputed from a second read of the row.  A row's bits depend on nothing
//           but the row and Cp.
//   fit     per entry the predicted class, max z and lse (T = 1); the valid entries compacted in (b, j) order (compact.h);
//           workgroup (c, s) adds p, max z and (max z)^2 of the rows of class c in chunk s of the compacted list, in list order,
//           to float64 partials; the chunks are added in chunk order and then to the running statistics.  The chunk bounds follow from the number of valid rows and C alone.  No floating-point atomics.
//
// Every row index is compared with its extent before a pointer is formed, every store index before the store; no call
// synchronises with the host or allocates, so all of them can be captured in a graph.
#include "common.h"
#include "feature_rows.h"
#include "wave_rows.h"

namespace {

constexpr int LO_MAX_CLASSES = 1024;
constexpr int LO_ROWS = 16;                                      // rows of a workgroup
constexpr int LO_WAVES = 4;
constexpr int LO_MAX_CHUNKS = 16;                                // row chunks of the fit partials
constexpr long long LO_PARTIAL_DOUBLES = 1ll << 18;              // the partials of all chunks stay below this many float64

struct LoArgs {
    const void* z; int bf16; long long bstride, astride;        // the logits: row (b, n) at b * bstride + n * astride (elements)
    int C, Cp;
    FoSel sel;                                                  // limit = N
    float T, gamma; int top_m;
    const float *logD, *kl_inf, *mu, *inv_sigma;                // [Cp][Cp], [Cp], [C], [C]; all null before a fit
    float *msp, *neg_entropy, *gen, *joint; long long* pred;
    float *kl, *sml; long long* kl_class;
    int use_min; float min_max;                                 // fit: rows with max z >= min_max only
    int* cls; float *mz, *lse; unsigned *list, *counts, *header; unsigned nblocks;
    double* partial; int S;
    long long* n_c; double *P_c, *a_c, *b_c;
};

// first logit of entry i = b * K + j, or null when the entry does not count
DEV const char* lo_rowp(const LoArgs& a, unsigned i) {
    unsigned b; long long an;
    if (!fo_select(a.sel, i, &b, &an)) return nullptr;
    return reinterpret_cast<const char*>(a.z) + ((long long)b * a.bstride + an * a.astride) * (a.bf16 ? 2 : 4);
}

template <int NC> struct LoSoft { float m, s, lse; int kstar; float e[NC], l[NC], p[NC]; };

// the softmax of the wave's row u (lane t: classes t + 64 i); e, l, p are 0 beyond C
template <int NC> DEV void lo_softmax(const float (&u)[NC], int C, int lane, LoSoft<NC>& r) {
    int ks;
    const float m = wr_argmax<NC>(u, C, lane, &ks);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        r.e[i] = lane + 64 * i < C ? expf(u[i] - m) : 0.f;
        s += r.e[i];
    }
    s = wave_reduce_sum(s);
    const float lse = m + logf(s);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const bool live = lane + 64 * i < C;
        r.l[i] = live ? u[i] - lse : 0.f;
        r.p[i] = live ? expf(r.l[i]) : 0.f;
    }
    r.m = m; r.s = s; r.lse = lse; r.kstar = ks;
}

template <int NC> DEV float lo_neg_entropy(const LoSoft<NC>& r) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) t += r.p[i] * r.l[i];           // (0 * 0 beyond C)
    return wave_reduce_sum(t);
}

DEV bool lo_less(float v, int c, float bv, int bc) { return v < bv || (v == bv && c < bc); }

template <int NC, int KC, int TM>
__global__ __launch_bounds__(LO_WAVES * 64) void lo_score_kernel(LoArgs a) {
    constexpr int PITCH = KC + 4;
    __shared__ __attribute__((aligned(16))) float ps[LO_ROWS * PITCH];
    __shared__ float ne1s[LO_ROWS], lse1s[LO_ROWS], bestv[LO_WAVES][LO_ROWS];
    __shared__ int bestc[LO_WAVES][LO_ROWS], rv[LO_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned row0 = (unsigned)blockIdx.x * LO_ROWS;
    const int C = a.C;
    const bool fitted = a.logD != nullptr;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr;
        const unsigned i = row0 + r;                            // the same for the whole wave
        const char* p = lo_rowp(a, i);
        if (!p) {
            if (fitted)
                for (int k = lane; k < KC; k += 64) ps[r * PITCH + k] = 0.f;
            if (lane == 0) {
                ne1s[r] = 0.f; lse1s[r] = 0.f; rv[r] = 0;
                if (i < a.sel.total) {
                    a.msp[i] = 0.f; a.neg_entropy[i] = 0.f; a.gen[i] = 0.f; a.joint[i] = 0.f; a.pred[i] = -1;
                    if (fitted) { a.kl[i] = 0.f; a.sml[i] = 0.f; a.kl_class[i] = -1; }
                }
            }
            continue;
        }
        float z[NC];
        wr_load<NC>(p, C, a.bf16, lane, z);
        LoSoft<NC> s;
        lo_softmax<NC>(z, C, lane, s);                          // T = 1
        const float maxz = s.m;
        float ne = lo_neg_entropy<NC>(s);
        if (lane == 0) lse1s[r] = s.lse;
        float je = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) je += lane + 64 * k < C ? wr_softplus(z[k]) : 0.f;
        je = wave_reduce_sum(je);
        if (fitted) {
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (lane + 64 * k < KC) ps[r * PITCH + lane + 64 * k] = s.p[k];     // zero beyond C
            if (lane == 0) ne1s[r] = ne;
        }
        if (lane == 0) rv[r] = 1;
        if (a.T != 1.f) {
#pragma unroll
            for (int k = 0; k < NC; ++k) z[k] = z[k] / a.T;
            lo_softmax<NC>(z, C, lane, s);
            ne = lo_neg_entropy<NC>(s);
        }
        const int ks = s.kstar;
        float so = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) so += lane + 64 * k == ks ? 0.f : s.e[k];
        so = wave_reduce_sum(so);
        const float qs = logf(so) - logf(s.s);
        unsigned key[NC];                                       // the top_m largest u, equal values: the lower class first
#pragma unroll
        for (int k = 0; k < NC; ++k) key[k] = fo_key(__float_as_uint(z[k]));
        const unsigned sel = wr_top<NC>(key, C, a.top_m, lane);
        float ge = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if ((sel >> k) & 1u) {
                const float q = lane + 64 * k == ks ? qs : log1pf(-s.p[k]);
                const float w = s.l[k] + q;
                ge += expf(a.gamma * w);
            }
        }
        ge = wave_reduce_sum(ge);
        if (lane == 0) {
            a.msp[i] = expf(s.m - s.lse);
            a.neg_entropy[i] = ne;
            a.gen[i] = -ge;
            a.joint[i] = je;
            const bool ok = ks >= 0 && ks < C;
            a.pred[i] = ok ? (long long)ks : -1;
            if (fitted) {
                const float d = maxz - (ok ? a.mu[ks] : 0.f);
                a.sml[i] = d * (ok ? a.inv_sigma[ks] : 0.f);
            }
        }
    }
    if (!fitted) return;                                        // (uniform over the workgroup)
    __syncthreads();
    const int Cp = a.Cp, ntiles = Cp / 16;
    f32x4 acc[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int k0 = 0; k0 < Cp; k0 += KC) {
        if (k0 > 0) {                                           // the next K-chunk of p, from a second read of the row
            __syncthreads();
#pragma unroll 1
            for (int rr = 0; rr < 4; ++rr) {
                const int r = wave * 4 + rr;
                const char* p = lo_rowp(a, row0 + r);
                const float lse = lse1s[r];
                for (int k = lane; k < KC; k += 64) {
                    const int kk = k0 + k;
                    float v = 0.f;
                    if (p && kk < C) { const float l = fo_ld(p, kk, a.bf16) - lse; v = expf(l); }
                    ps[r * PITCH + k] = v;
                }
            }
            __syncthreads();
        }
        const int kend = Cp - k0 < KC ? Cp - k0 : KC;
#pragma unroll 1
        for (int kc = 0; kc < kend; kc += 16) {
            const Frag<float> fa = ld_frag<float>(ps + r16 * PITCH + kc + g * 4);
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                const int tile = wave + LO_WAVES * t;
                if (tile < ntiles) {
                    const Frag<float> fb = ld_frag<float>(a.logD + (long long)(tile * 16 + r16) * Cp + k0 + kc + g * 4);
                    mma_chunk(fa, fb, acc[t]);
                }
            }
        }
    }
    // a lane holds kl of class 16 tile + (lane & 15) for rows 4 (lane >> 4) + 0 .. 3
    float bv[4]; int bc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { bv[q] = __builtin_inff(); bc[q] = WR_NONE; }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        const int tile = wave + LO_WAVES * t;
        if (tile < ntiles) {
            const int c = tile * 16 + r16;
            const float inf = a.kl_inf[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = ne1s[4 * g + q] - acc[t][q];
                const float v = d + inf;
                if (lo_less(v, c, bv[q], bc[q])) { bv[q] = v; bc[q] = c; }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float ov = __shfl_xor(bv[q], o, 64);
            const int oc = __shfl_xor(bc[q], o, 64);
            if (lo_less(ov, oc, bv[q], bc[q])) { bv[q] = ov; bc[q] = oc; }
        }
    if (r16 == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { bestv[wave][4 * g + q] = bv[q]; bestc[wave][4 * g + q] = bc[q]; }
    }
    __syncthreads();
    if (tid < LO_ROWS) {
        const unsigned i = row0 + tid;
        if (i < a.sel.total && rv[tid]) {
            float v = bestv[0][tid]; int c = bestc[0][tid];
            for (int w = 1; w < LO_WAVES; ++w)
                if (lo_less(bestv[w][tid], bestc[w][tid], v, c)) { v = bestv[w][tid]; c = bestc[w][tid]; }
            a.kl[i] = -v;
            a.kl_class[i] = c == WR_NONE ? -1 : (long long)c;
        }
    }
}

// ---- fit ---------------------------------------------------------------------------------------------------------------------
// per entry: the predicted class (-1: the entry does not count), max z and the log-sum-exp at T = 1
template <int NC>
__global__ __launch_bounds__(LO_WAVES * 64) void lo_fit_rows_kernel(LoArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const unsigned i = (unsigned)blockIdx.x * LO_ROWS + wave * 4 + rr;
        if (i >= a.sel.total) continue;
        const char* p = lo_rowp(a, i);
        int cls = -1; float mz = 0.f, lse = 0.f;
        if (p) {
            float z[NC];
            wr_load<NC>(p, C, a.bf16, lane, z);
            LoSoft<NC> s;
            lo_softmax<NC>(z, C, lane, s);
            mz = s.m; lse = s.lse;
            int ks = s.kstar;
            if (a.T != 1.f) {                                   // the predicted class is the argmax of u = z / T, as in the score
#pragma unroll
                for (int k = 0; k < NC; ++k) z[k] = z[k] / a.T;
                wr_argmax<NC>(z, C, lane, &ks);
            }
            if (ks >= 0 && ks < C && (!a.use_min || mz >= a.min_max)) cls = ks;
        }
        if (lane == 0) { a.cls[i] = cls; a.mz[i] = mz; a.lse[i] = lse; }
    }
}

DEV bool cp_keep(const LoArgs& a, unsigned i) { return i < a.sel.total && a.cls[i] >= 0; }
DEV unsigned cp_begin(const LoArgs&) { return 0u; }
DEV void cp_finish(const LoArgs& a, unsigned, unsigned total) { a.header[0] = fo_min(total, a.sel.total); }

// blockIdx.x = class c, blockIdx.y = chunk s of the compacted list: partial[s][c] = {sum p [C], sum max z, sum (max z)^2, n} over
// the chunk's rows of class c, in list order
__global__ __launch_bounds__(256) void lo_fit_sum_kernel(LoArgs a) {
    __shared__ int match[FO_THREADS];
    const int tid = threadIdx.x, C = a.C;
    const int c = blockIdx.x, s = blockIdx.y;
    const unsigned V = fo_min(a.header[0], a.sel.total);
    const unsigned len = (V + (unsigned)a.S - 1) / (unsigned)a.S;
    const unsigned lo = fo_min((unsigned)s * len, V), hi = fo_min(lo + len, V);
    double acc[LO_MAX_CLASSES / FO_THREADS];
#pragma unroll
    for (int q = 0; q < LO_MAX_CLASSES / FO_THREADS; ++q) acc[q] = 0.0;
    double sa = 0.0, sb = 0.0, n = 0.0;                         // n <= 2^27: exact
    for (unsigned base = lo; base < hi; base += FO_THREADS) {
        const unsigned v = base + tid;
        int e = -1;
        if (v < hi) {
            const unsigned i = a.list[v];
            if (i < a.sel.total && a.cls[i] == c) e = (int)i;
        }
        match[tid] = e;
        __syncthreads();
        for (int j = 0; j < FO_THREADS; ++j) {
            const int i = match[j];                             // the same for the whole workgroup
            if (i < 0) continue;
            const char* p = lo_rowp(a, (unsigned)i);
            if (!p) continue;
            const float lse = a.lse[i];
#pragma unroll
            for (int q = 0; q < LO_MAX_CLASSES / FO_THREADS; ++q) {
                const int k = tid + FO_THREADS * q;
                if (k < C) { const float l = fo_ld(p, k, a.bf16) - lse; acc[q] += (double)expf(l); }
            }
            const double mz = (double)a.mz[i];
            sa += mz; sb += mz * mz; n += 1.0;
        }
        __syncthreads();
    }
    double* o = a.partial + ((long long)s * C + c) * (C + 3);
#pragma unroll
    for (int q = 0; q < LO_MAX_CLASSES / FO_THREADS; ++q) {
        const int k = tid + FO_THREADS * q;
        if (k < C) o[k] = acc[q];
    }
    if (tid == 0) { o[C] = sa; o[C + 1] = sb; o[C + 2] = n; }
}

// blockIdx.x = class c: the chunks in chunk order, then onto the running statistics
__global__ __launch_bounds__(256) void lo_fit_reduce_kernel(LoArgs a) {
    const int C = a.C, c = blockIdx.x;
    for (int k = threadIdx.x; k < C + 3; k += FO_THREADS) {
        double t = 0.0;
        for (int s = 0; s < a.S; ++s) t += a.partial[((long long)s * C + c) * (C + 3) + k];
        if (k < C) a.P_c[(long long)c * C + k] += t;
        else if (k == C) a.a_c[c] += t;
        else if (k == C + 1) a.b_c[c] += t;
        else a.n_c[c] += (long long)t;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct LoLayout { long long cls, mz, lse, list, counts, header, partial, bytes; unsigned nblocks; int S; };

int lo_chunks(int C) {
    const long long s = LO_PARTIAL_DOUBLES / ((long long)C * (C + 3));
    return (int)(s < 1 ? 1 : (s > LO_MAX_CHUNKS ? LO_MAX_CHUNKS : s));
}

bool lo_layout(long long rows, int C, LoLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS || C < 1 || C > LO_MAX_CLASSES) return false;
    L->nblocks = (unsigned)((rows + FO_TILE - 1) / FO_TILE);
    L->S = lo_chunks(C);
    FoCarve ws;
    L->cls = ws.take(rows * 4);
    L->mz = ws.take(rows * 4);
    L->lse = ws.take(rows * 4);
    L->list = ws.take(rows * 4);
    L->counts = ws.take((long long)L->nblocks * 4);
    L->header = ws.take(256);
    L->partial = ws.take((long long)L->S * C * (C + 3) * 8);
    L->bytes = ws.at;
    return true;
}

// the arguments both entry points share; false: refuse
bool lo_args(int dtype, const void* logits, long long image_stride, long long anchor_stride, int C, int B, long long N, long long K,
             const long long* anchor_index, const void* count, int count_is_int64, float temperature, LoArgs* a) {
    if ((dtype != EFFDET_F32 && dtype != EFFDET_BF16) || !logits || image_stride < 0 || anchor_stride < 0) return false;
    if (C < 1 || C > LO_MAX_CLASSES || N > (1ll << 31) || !(temperature > 0.f) || !(temperature < __builtin_inff())) return false;
    *a = LoArgs{};
    if (!fo_sel(B, K, anchor_index, count, count_is_int64, N, &a->sel)) return false;
    a->z = logits; a->bf16 = dtype == EFFDET_BF16; a->bstride = image_stride; a->astride = anchor_stride;
    a->C = C; a->Cp = (C + 15) / 16 * 16;
    a->T = temperature;
    return true;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_logit_ood_workspace_bytes(long long rows, int C) {
    LoLayout L;
    return lo_layout(rows, C, &L) ? L.bytes : EFFDET_EINVAL;
}

extern "C" int effdet_logit_ood_score(void* stream, int dtype, const void* logits, long long image_stride, long long anchor_stride,
                                      int C, int B, long long N, long long K, const long long* anchor_index, const void* count,
                                      int count_is_int64, float temperature, float gamma, int top_m, const float* log_d,
                                      const float* kl_inf, const float* mu, const float* inv_sigma, float* msp, float* neg_entropy,
                                      float* gen, float* joint_energy, long long* predicted_class, float* kl_matching,
                                      long long* kl_class, float* standardized) {
    LoArgs a;
    if (!lo_args(dtype, logits, image_stride, anchor_stride, C, B, N, K, anchor_index, count, count_is_int64, temperature, &a))
        return EFFDET_EINVAL;
    if (!(gamma == gamma) || gamma - gamma != 0.f || top_m < 1) return EFFDET_EINVAL;
    if (!msp || !neg_entropy || !gen || !joint_energy || !predicted_class) return EFFDET_EINVAL;
    const int fitted = (log_d ? 1 : 0) + (kl_inf ? 1 : 0) + (mu ? 1 : 0) + (inv_sigma ? 1 : 0) + (kl_matching ? 1 : 0) + (kl_class ? 1 : 0) +
                       (standardized ? 1 : 0);
    if (fitted != 0 && fitted != 7) return EFFDET_EINVAL;       // the fitted parameters and their outputs come together
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    a.gamma = gamma; a.top_m = top_m;
    a.logD = log_d; a.kl_inf = kl_inf; a.mu = mu; a.inv_sigma = inv_sigma;
    a.msp = msp; a.neg_entropy = neg_entropy; a.gen = gen; a.joint = joint_energy; a.pred = predicted_class;
    a.kl = kl_matching; a.kl_class = kl_class; a.sml = standardized;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a.sel.total + LO_ROWS - 1) / LO_ROWS), block(LO_WAVES * 64);
    wr_for_classes(a.Cp, [&](auto nc) {                         // p passes through LDS in K-chunks of at most 512 classes
        constexpr int NC = decltype(nc)::value, KC = 64 * NC < 512 ? 64 * NC : 512;
        hipLaunchKernelGGL((lo_score_kernel<NC, KC, NC>), grid, block, 0, st, a);
    });
    return effdet_check_launch();
}

extern "C" int effdet_logit_ood_fit(void* stream, int dtype, const void* logits, long long image_stride, long long anchor_stride, int C,
                                    int B, long long N, long long K, const long long* anchor_index, const void* count,
                                    int count_is_int64, float temperature, int use_min, float min_max_logit, long long* n_c,
                                    double* P_c, double* a_c, double* b_c, void* workspace, long long workspace_bytes) {
    LoArgs a;
    if (!lo_args(dtype, logits, image_stride, anchor_stride, C, B, N, K, anchor_index, count, count_is_int64, temperature, &a))
        return EFFDET_EINVAL;
    LoLayout L;
    if (!lo_layout((long long)B * K, C, &L)) return EFFDET_EINVAL;
    if (use_min && !(min_max_logit == min_max_logit)) return EFFDET_EINVAL;
    if (!n_c || !P_c || !a_c || !b_c || !workspace || workspace_bytes < L.bytes) return EFFDET_EINVAL;
    EFFDET_ENTER();
    char* ws = reinterpret_cast<char*>(workspace);
    a.use_min = use_min ? 1 : 0; a.min_max = min_max_logit;
    a.cls = reinterpret_cast<int*>(ws + L.cls); a.mz = reinterpret_cast<float*>(ws + L.mz); a.lse = reinterpret_cast<float*>(ws + L.lse);
    a.list = reinterpret_cast<unsigned*>(ws + L.list); a.counts = reinterpret_cast<unsigned*>(ws + L.counts);
    a.header = reinterpret_cast<unsigned*>(ws + L.header); a.nblocks = L.nblocks;
    a.partial = reinterpret_cast<double*>(ws + L.partial); a.S = L.S;
    a.n_c = n_c; a.P_c = P_c; a.a_c = a_c; a.b_c = b_c;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a.sel.total + LO_ROWS - 1) / LO_ROWS), block(LO_WAVES * 64);
    wr_for_classes(a.Cp, [&](auto nc) { hipLaunchKernelGGL(lo_fit_rows_kernel<decltype(nc)::value>, grid, block, 0, st, a); });
    hipLaunchKernelGGL(fo_count_kernel<LoArgs>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_base_kernel<LoArgs>, dim3(1), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_write_index_kernel<LoArgs>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(lo_fit_sum_kernel, dim3(C, a.S), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(lo_fit_reduce_kernel, dim3(C), dim3(FO_THREADS), 0, st, a);
    return effdet_check_launch();
}
