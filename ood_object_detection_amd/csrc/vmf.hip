// The von Mises-Fisher hyperspherical OOD head on the device (SIREN, Du et al. 2022): the partition function of the
// vMF density per class, the ordered prototype update, the vMF log-likelihood loss forward and backward, the scores, and the gather
// of tower rows that feeds the head's MLP at inference.
//
//   U [B][P][d] float32 is the MLP's embedding of every cell; entry i = (b, j) of a dense [B, K = A P] label map counts when its
//   label y lies in [0, C) (FoSel / FoClasses) and the row u of its cell p = j / A holds finite values only.
//     n = max(sqrt(sum_k u_k^2), 1e-12), r = u / n       the sum: lane t adds elements t, t + 64, .. ascending, then the xor tree
//     kappa_c = float32(exp(clamp(theta_c, log 2^-7, log 2^13))), nu = d / 2 - 1
//     logZ_c = nu log kappa_c - (d / 2) log(2 pi) - log I_nu(kappa_c),  A_c = I_{nu+1}(kappa_c) / I_nu(kappa_c)      (float64)
//     l_c = float32(logZ_c) + kappa_c * (mu_c . r)        over the valid classes; the dot product adds k = 0 .. d - 1 in order
//     loss_i = logsumexp_c l_c - l_y, p = softmax l, g_c = (p_c - [c = y]) * float32(1 / max(m, 1))
//     d theta_c = kappa_c sum_i g_ic ((mu_c . r_i) - A_c)  (float64 terms and sum; 0 where the clamp is active)
//     G = sum_c (g_c kappa_c) mu_c (c ascending), du = (G - (G . r) r) / n;  dU of a cell: its counted anchors' du added ascending
//   partition  a thread per class, float64: I_nu(x) = (x / 2)^nu sum_k q^k / (k! Gamma(nu + k + 1)), q = x^2 / 4, as a series of
//              positive terms relative to its largest term k0 (the root of k (nu + k) = q), upwards and then downwards by the term
//              ratio until a term falls below 2^-60 of the sum; A = (2 / x) sum_k k t_k / sum_k t_k (the derivative of the series).
//   flags      a thread per entry: the label, -1 not counted, -2 a non-finite row, -3 its class has no prototype yet; then the
//              ordered compaction of compact.h puts the counted entries in (b, j) order and leaves their number m on the device.
//   update     one wave per class walks the list, 64 entries a round, and applies its own rows in order:
//              v = alpha * mu + (1 - alpha) * r, mu = v / max(|v|, 1e-12), the norm summed like n.  At most `limit` rows.
//   loss       a wave takes the first counted anchor of a cell and with it the cell's other counted anchors (they are neighbours in
//              the list): r, the logits and the softmax once, then g, G and du per anchor.  Wave w of W takes list positions w, w + W,
//              .. ascending and keeps float64 sums per class; the final kernel adds the W partial rows of a class: thread t of 256 its rows
//              t, t + 256, .. ascending, then the tree of compact.h.
//   score      a wave per selected row (anchor_index / count, or every cell): max_c l_c, the lowest class that attains it, max_c
//              mu_c . r, and optionally r itself.
// No floating-point atomics, no allocation, no host synchronisation; the order of every sum follows from B * K alone.  Every index
// is compared with its extent before a pointer is formed.
#include "common.h"
#include "feature_rows.h"
#include "wave_rows.h"

namespace {

constexpr int VM_MAX_CLASSES = 1024, VM_MAX_DIM = 256;
constexpr int VM_ND = VM_MAX_DIM / 64;                          // registers of a lane for one row of d values
constexpr int VM_WAVES = 4;
constexpr int VM_MAX_GROUPS = 1024;                             // workgroups of the loss kernel: four waves a SIMD on 256 CUs
constexpr int VM_SCORE_ROWS = 16;                               // rows of a score workgroup
constexpr int VM_MAX_TERMS = 1 << 14;                           // of one direction of the Bessel series (852 suffice at kappa 2^13)
constexpr float VM_EPS = 1e-12f;
constexpr float VM_THETA_LO = -4.852030263919617f, VM_THETA_HI = 9.010913347279288f;       // log 2^-7, log 2^13

// ---- the partition function -----------------------------------------------------------------------------------------------------
// log I_nu(x) and I_{nu+1}(x) / I_nu(x) for x > 0, nu >= 0
DEV void vm_bessel(double nu, double x, double* log_i, double* ratio) {
    const double q = 0.25 * x * x;
    const double k0 = floor(2.0 * q / (nu + sqrt(nu * nu + x * x)));       // the largest term: k (nu + k) <= q
    const double log_t0 = k0 * log(q) - lgamma(k0 + 1.0) - lgamma(nu + k0 + 1.0);
    const double tiny = 8.673617379884035e-19;                  // 2^-60
    double s = 1.0, sk = k0, t = 1.0;
    for (int n = 1; n <= VM_MAX_TERMS; ++n) {                   // upwards: t_k = t_{k-1} q / (k (nu + k))
        const double k = k0 + (double)n;
        t = t * (q / (k * (nu + k)));
        s += t; sk += t * k;
        if (t < tiny * s) break;
    }
    t = 1.0;
    for (int n = 1; n <= VM_MAX_TERMS; ++n) {                   // downwards: t_k = t_{k+1} (k + 1) (nu + k + 1) / q
        const double k = k0 - (double)n;
        if (k < 0.0) break;
        t = t * (((k + 1.0) * (nu + k + 1.0)) / q);
        s += t; sk += t * k;
        if (t < tiny * s) break;
    }
    *log_i = nu * log(0.5 * x) + log_t0 + log(s);
    *ratio = (2.0 / x) * (sk / s);
}

__global__ __launch_bounds__(256) void vm_partition_kernel(const float* theta, int C, int d, float* kappa, float* logz, double* logz64,
                                                           double* ratio, int* clamped) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float t = theta[c];
    const bool inside = t >= VM_THETA_LO && t <= VM_THETA_HI;   // (false for a NaN, which the clamp sends to the lower end)
    const float tc = fminf(fmaxf(t, VM_THETA_LO), VM_THETA_HI);
    const float kf = (float)exp((double)tc);
    const double x = (double)kf, nu = 0.5 * (double)d - 1.0;
    double li, a;
    vm_bessel(nu, x, &li, &a);
    const double lz = nu * log(x) - (nu + 1.0) * 1.8378770664093453 - li;      // log(2 pi)
    kappa[c] = kf; logz[c] = (float)lz; logz64[c] = lz; ratio[c] = a; clamped[c] = inside ? 0 : 1;
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------
struct VmRows {
    const float* U; unsigned P; int A, d;                       // [B][P][d]
    FoSel sel; FoClasses cls;                                   // K = A * P, no anchor index, no count
    const int* valid; int need_valid;
    int* lab;                                                   // workspace [total]: the label, or -1 / -2 / -3
    unsigned *counts, nblocks, *list, *m, *skipped;             // compaction; skipped [nblocks]: non-finite rows of a tile
};
DEV bool cp_keep(const VmRows& a, unsigned i) { return i < a.sel.total && a.lab[i] >= 0; }
DEV unsigned cp_begin(const VmRows&) { return 0u; }
DEV void cp_finish(const VmRows& a, unsigned, unsigned total) { a.m[0] = fo_min(total, a.sel.total); }

// the embedding row of entry e (< total)
DEV const float* vm_row(const VmRows& a, unsigned e) {
    const unsigned b = e / a.sel.K, j = e - b * a.sel.K;
    return a.U + ((long long)b * a.P + j / (unsigned)a.A) * a.d;
}

__global__ __launch_bounds__(256) void vm_flag_kernel(VmRows a) {
    __shared__ unsigned sh[FO_THREADS];
    const int tid = threadIdx.x;
    unsigned skip = 0;
    for (int r = 0; r < FO_ITEMS; ++r) {
        const unsigned i = (unsigned)blockIdx.x * FO_TILE + r * FO_THREADS + tid;
        unsigned b; long long an;
        if (!fo_select(a.sel, i, &b, &an)) { if (i < a.sel.total) a.lab[i] = -1; continue; }
        int lab = fo_class(a.cls, b, (unsigned)an);
        if (lab >= 0) {
            if (a.need_valid && !a.valid[lab]) lab = -3;
            else {
                const float* u = vm_row(a, i);
                bool fin = true;
                for (int k = 0; k < a.d; ++k) { const float v = u[k]; fin = fin && (v - v == 0.f); }
                if (!fin) { lab = -2; ++skip; }
            }
        }
        a.lab[i] = lab;
    }
    const unsigned tot = fo_block_sum<unsigned>(skip, sh, tid);
    if (tid == 0) a.skipped[blockIdx.x] = tot;
}

// u -> u / max(|u|, EPS) in place; the norm
DEV float vm_unit(float (&u)[VM_ND], int lane) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VM_ND; ++i) s += u[i] * u[i];           // (zero beyond d)
    s = wave_reduce_sum(s);
    const float n = fmaxf(sqrtf(s), VM_EPS);
#pragma unroll
    for (int i = 0; i < VM_ND; ++i) u[i] = u[i] / n;
    return n;
}

__global__ __launch_bounds__(64) void vm_update_kernel(VmRows a, float alpha, long long limit, float* proto, int* valid) {
    __shared__ unsigned she[64];
    const int lane = threadIdx.x, c = blockIdx.x, d = a.d;
    const unsigned m = fo_min(a.m[0], a.sel.total);
    float mu[VM_ND];
    wr_load<VM_ND>(reinterpret_cast<const char*>(proto + (long long)c * d), d, 0, lane, mu);
    const float beta = 1.f - alpha;
    long long taken = 0;
    bool done = false;
    for (unsigned base = 0; base < m && !done; base += 64) {    // (uniform over the wave)
        const unsigned q = base + lane;
        const unsigned e = q < m ? a.list[q] : 0u;
        const bool match = q < m && e < a.sel.total && a.lab[e] == c;
        unsigned long long bal = __ballot(match);
        she[lane] = e;
        __syncthreads();
        while (bal != 0ull && !done) {
            const int src = __builtin_ctzll(bal);
            bal &= bal - 1ull;
            float r[VM_ND];
            wr_load<VM_ND>(reinterpret_cast<const char*>(vm_row(a, she[src])), d, 0, lane, r);
            vm_unit(r, lane);
#pragma unroll
            for (int i = 0; i < VM_ND; ++i) mu[i] = alpha * mu[i] + beta * r[i];
            vm_unit(mu, lane);
            ++taken;
            done = limit > 0 && taken >= limit;
        }
        __syncthreads();
    }
    if (taken > 0) {
#pragma unroll
        for (int i = 0; i < VM_ND; ++i)
            if (lane + 64 * i < d) proto[(long long)c * d + lane + 64 * i] = mu[i];
        if (lane == 0) valid[c] = 1;
    }
}

// ---- logits ---------------------------------------------------------------------------------------------------------------------
struct VmHead { int C, d; const float *proto, *muT, *kappa, *logz; const int* valid; };        // muT [d][C]: workspace

__global__ __launch_bounds__(256) void vm_transpose_kernel(const float* proto, float* muT, int C, int d) {
    const int i = blockIdx.x * 256 + threadIdx.x;               // element (j, c) of muT
    if (i >= C * d) return;
    const int j = i / C, c = i - j * C;
    muT[i] = proto[(long long)c * d + j];
}

// the classes lane, lane + 64, .. of this lane from the unit row rs (LDS): dot = mu_c . r, l = logZ_c + kappa_c dot; a class that
// is not valid gets -inf / -inf.  -> bit k: class lane + 64 k is valid
template <int NC> DEV unsigned vm_logits(const VmHead& h, const float* rs, int lane, float (&l)[NC], float (&dot)[NC]) {
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const int c = lane + 64 * k;
        const bool ok = c < h.C && h.valid[c] != 0;
        float acc = 0.f;
        if (ok) {
#pragma unroll 8
            for (int j = 0; j < h.d; ++j) acc += h.muT[(long long)j * h.C + c] * rs[j];      // (unrolled: the loads of eight steps in flight)
            live |= 1u << k;
        }
        dot[k] = ok ? acc : -__builtin_inff();
        l[k] = ok ? h.logz[c] + h.kappa[c] * acc : -__builtin_inff();
    }
    return live;
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------
struct VmLoss {
    VmRows r; VmHead h;
    const double* ratio; const int* clamped;
    double* partial; unsigned nwaves;                            // [nwaves][C + 2]
    float *loss, *dU, *dtheta; double* stats;
    long long du_elems;
};

__global__ __launch_bounds__(256) void vm_zero_kernel(float* p, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

template <int NC> __global__ __launch_bounds__(VM_WAVES * 64) void vm_loss_kernel(VmLoss a) {
    __shared__ float rs[VM_WAVES][VM_MAX_DIM];
    __shared__ float wsh[VM_WAVES][VM_MAX_CLASSES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.h.C, d = a.h.d;
    const unsigned wid = (unsigned)blockIdx.x * VM_WAVES + wave, nw = a.nwaves;
    const unsigned m = fo_min(a.r.m[0], a.r.sel.total), A = (unsigned)a.r.A;
    const float coef = (float)(1.0 / (double)(m < 1u ? 1u : m));
    double acc[NC], loss_acc = 0.0, dot_acc = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (unsigned q = wid; q < m; q += nw) {                    // (uniform over the wave)
        const unsigned e = a.r.list[q];
        if (e >= a.r.sel.total) continue;
        const unsigned cell = e / A;                            // = b * P + p
        if (q > 0 && a.r.list[q - 1] / A == cell) continue;     // the cell's first counted anchor takes the others with it
        float r[VM_ND], l[NC], dot[NC];
        wr_load<VM_ND>(reinterpret_cast<const char*>(vm_row(a.r, e)), d, 0, lane, r);
        const float n = vm_unit(r, lane);
        __builtin_amdgcn_wave_barrier();                        // the lanes have read the last row before one writes this one
#pragma unroll
        for (int i = 0; i < VM_ND; ++i) rs[wave][lane + 64 * i] = r[i];
        __builtin_amdgcn_wave_barrier();
        const unsigned live = vm_logits<NC>(a.h, rs[wave], lane, l, dot);
        float mx = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < NC; ++k) mx = fmaxf(mx, l[k]);
        mx = wave_reduce_max(mx);
        float s = 0.f, p[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { p[k] = ((live >> k) & 1u) ? expf(l[k] - mx) : 0.f; s += p[k]; }
        s = wave_reduce_sum(s);
        const float lse = mx + logf(s);
#pragma unroll
        for (int k = 0; k < NC; ++k) p[k] = p[k] / s;
        float du[VM_ND];
#pragma unroll
        for (int i = 0; i < VM_ND; ++i) du[i] = 0.f;
#pragma unroll 1
        for (unsigned qq = q; qq < m; ++qq) {
            const unsigned ee = a.r.list[qq];
            if (ee >= a.r.sel.total || ee / A != cell) break;
            const int y = a.r.lab[ee];
            float ly = -__builtin_inff(), dy = -__builtin_inff();
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int c = lane + 64 * k;
                if (c >= C) continue;
                float w = 0.f;
                if ((live >> k) & 1u) {
                    const float g = (p[k] - (c == y ? 1.f : 0.f)) * coef;
                    w = g * a.h.kappa[c];
                    acc[k] += (double)g * ((double)dot[k] - a.ratio[c]);
                    if (c == y) { ly = l[k]; dy = dot[k]; }
                }
                wsh[wave][c] = w;
            }
            __builtin_amdgcn_wave_barrier();
            ly = wave_reduce_max(ly); dy = wave_reduce_max(dy);
            loss_acc += (double)(lse - ly);
            dot_acc += (double)dy;
            float G[VM_ND];
#pragma unroll
            for (int i = 0; i < VM_ND; ++i) G[i] = 0.f;
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                if (!a.h.valid[c]) continue;                    // (what a class without a prototype holds cannot matter)
                const float w = wsh[wave][c];
#pragma unroll
                for (int i = 0; i < VM_ND; ++i)
                    if (lane + 64 * i < d) G[i] += w * a.h.proto[(long long)c * d + lane + 64 * i];
            }
            float gr = 0.f;
#pragma unroll
            for (int i = 0; i < VM_ND; ++i) gr += G[i] * r[i];
            gr = wave_reduce_sum(gr);
#pragma unroll
            for (int i = 0; i < VM_ND; ++i) du[i] += (G[i] - gr * r[i]) / n;
        }
#pragma unroll
        for (int i = 0; i < VM_ND; ++i) {
            const long long at = (long long)cell * d + lane + 64 * i;
            if (lane + 64 * i < d && at < a.du_elems) a.dU[at] = du[i];
        }
    }
    if (wid < nw) {
        double* out = a.partial + (long long)wid * (C + 2);
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if (lane + 64 * k < C) out[lane + 64 * k] = acc[k];
        if (lane == 0) { out[C] = loss_acc; out[C + 1] = dot_acc; }
    }
}

// workgroup c: column c of the partial rows - thread t adds rows t, t + 256, .. ascending, then the tree of compact.h; the last
// workgroup (blockIdx.x = C + 2) the statistics
__global__ __launch_bounds__(256) void vm_final_kernel(VmLoss a) {
    __shared__ double shd[FO_THREADS];
    __shared__ unsigned sh[FO_THREADS];
    const int tid = threadIdx.x, C = a.h.C;
    const int col = blockIdx.x;
    const unsigned m = fo_min(a.r.m[0], a.r.sel.total);
    const double dm = (double)(m < 1u ? 1u : m);
    if (col < C + 2) {
        double t = 0.0;
        for (unsigned w = tid; w < a.nwaves; w += FO_THREADS) t += a.partial[(long long)w * (C + 2) + col];
        t = fo_block_sum<double>(t, shd, tid);
        if (tid != 0) return;
        if (col < C) a.dtheta[col] = a.clamped[col] ? 0.f : (float)((double)a.h.kappa[col] * t);
        else if (col == C) { a.loss[0] = (float)(t / dm); a.stats[6] = t / dm; }
        else a.stats[3] = t / dm;
        return;
    }
    unsigned skip = 0, nvalid = 0;
    for (unsigned k = tid; k < a.r.nblocks; k += FO_THREADS) skip += a.r.skipped[k];
    for (int c = tid; c < C; c += FO_THREADS) nvalid += a.h.valid[c] != 0 ? 1u : 0u;
    skip = fo_block_sum<unsigned>(skip, sh, tid);
    nvalid = fo_block_sum<unsigned>(nvalid, sh, tid);
    if (tid != 0) return;
    double ks = 0.0, kmax = 0.0;
    for (int c = 0; c < C; ++c) { const double k = (double)a.h.kappa[c]; ks += k; kmax = k > kmax ? k : kmax; }
    a.stats[0] = (double)m; a.stats[1] = (double)skip; a.stats[2] = (double)nvalid;
    a.stats[4] = ks / (double)C; a.stats[5] = kmax; a.stats[7] = 0.0;
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
struct VmScore {
    const float* U; unsigned P; int A, gathered; FoSel sel; VmHead h;
    float* vmf; long long* cls; float* cosine; float* rows;
};

template <int NC> __global__ __launch_bounds__(VM_WAVES * 64) void vm_score_kernel(VmScore a) {
    __shared__ float rs[VM_WAVES][VM_MAX_DIM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.h.C, d = a.h.d;
#pragma unroll 1
    for (int rr = 0; rr < VM_SCORE_ROWS / VM_WAVES; ++rr) {
        const unsigned i = (unsigned)blockIdx.x * VM_SCORE_ROWS + wave * (VM_SCORE_ROWS / VM_WAVES) + rr;      // the same for the whole wave
        if (i >= a.sel.total) continue;
        unsigned b; long long an;
        const bool ok = fo_select(a.sel, i, &b, &an);
        float best = 0.f, cosb = 0.f, r[VM_ND];
        long long kc = -1;
#pragma unroll
        for (int k = 0; k < VM_ND; ++k) r[k] = 0.f;
        if (ok) {
            const float* u = a.gathered ? a.U + (long long)i * d : a.U + ((long long)b * a.P + (unsigned)(an / a.A)) * d;
            wr_load<VM_ND>(reinterpret_cast<const char*>(u), d, 0, lane, r);
            bool bad = false;
#pragma unroll
            for (int k = 0; k < VM_ND; ++k) bad = bad || !(r[k] - r[k] == 0.f);
            const bool nonfinite = __ballot(bad) != 0ull;
            vm_unit(r, lane);
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < VM_ND; ++k) rs[wave][lane + 64 * k] = r[k];
            __builtin_amdgcn_wave_barrier();
            float l[NC], dot[NC];
            const unsigned live = vm_logits<NC>(a.h, rs[wave], lane, l, dot);
            const bool any = __ballot(live != 0u) != 0ull;
            int ks;
            const float mx = wr_argmax<NC>(l, C, lane, &ks);
            float cm = -__builtin_inff();
#pragma unroll
            for (int k = 0; k < NC; ++k) cm = fmaxf(cm, dot[k]);
            cm = wave_reduce_max(cm);
            if (nonfinite) { best = __builtin_nanf(""); cosb = best; }
            else if (any && ks >= 0 && ks < C) { best = mx; cosb = cm; kc = ks; }
        }
        if (lane == 0) { a.vmf[i] = best; a.cls[i] = kc; a.cosine[i] = cosb; }
        if (a.rows) {
#pragma unroll
            for (int k = 0; k < VM_ND; ++k)
                if (lane + 64 * k < d) a.rows[(long long)i * d + lane + 64 * k] = r[k];
        }
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------
struct VmGather { FoLevels L; FoSel sel; int A, F; float* out; };

__global__ __launch_bounds__(VM_WAVES * 64) void vm_gather_kernel(VmGather a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned i = (unsigned)blockIdx.x * VM_WAVES + wave;
    if (i >= a.sel.total) return;
    const char* p = fo_sel_row(a.L, a.sel, a.A, i);             // the same for the whole wave
    for (int k = lane; k < a.F; k += 64) a.out[(long long)i * a.F + k] = p ? fo_ld(p, k, a.L.bf16) : 0.f;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct VmLayout { long long lab, counts, skipped, list, m, muT, partial, bytes; unsigned nblocks, ngroups; };

bool vm_layout(long long rows, int C, int d, VmLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS || C < 1 || C > VM_MAX_CLASSES || d < 2 || d > VM_MAX_DIM) return false;
    L->nblocks = (unsigned)((rows + FO_TILE - 1) / FO_TILE);
    const long long groups = (rows + 63) / 64;
    L->ngroups = (unsigned)(groups < VM_MAX_GROUPS ? groups : VM_MAX_GROUPS);
    FoCarve ws;
    L->lab = ws.take(rows * 4);
    L->counts = ws.take((long long)L->nblocks * 4);
    L->skipped = ws.take((long long)L->nblocks * 4);
    L->list = ws.take(rows * 4);
    L->m = ws.take(256);
    L->muT = ws.take((long long)C * d * 4);
    L->partial = ws.take((long long)L->ngroups * VM_WAVES * (C + 2) * 8);
    L->bytes = ws.at;
    return true;
}

bool vm_finite(float v) { return v - v == 0.f; }

// the dense label map of a call: U [B][P][d], labels [B][K = A P]
bool vm_rows(const float* U, int B, long long P, int A, int d, const void* classes, int classes_dtype, long long classes_pitch,
             long long classes_stride, long long class_offset, int C, void* workspace, long long workspace_bytes, VmRows* r,
             VmLayout* L) {
    if (!U || B < 1 || P < 1 || A < 1 || P > (1ll << 31) || (long long)B * P > (1ll << 31)) return false;
    if (A > FO_MAX_ROWS || P * A > FO_MAX_ROWS) return false;
    if (!vm_layout((long long)B * P * A, C, d, L) || !workspace || workspace_bytes < L->bytes) return false;
    *r = VmRows{};
    if (!fo_sel(B, P * A, nullptr, nullptr, 0, P * A, &r->sel)) return false;
    if (!fo_classes(classes, classes_dtype, classes_pitch, classes_stride, class_offset, C, &r->cls)) return false;
    char* ws = reinterpret_cast<char*>(workspace);
    r->U = U; r->P = (unsigned)P; r->A = A; r->d = d;
    r->lab = reinterpret_cast<int*>(ws + L->lab);
    r->counts = reinterpret_cast<unsigned*>(ws + L->counts); r->nblocks = L->nblocks;
    r->skipped = reinterpret_cast<unsigned*>(ws + L->skipped);
    r->list = reinterpret_cast<unsigned*>(ws + L->list);
    r->m = reinterpret_cast<unsigned*>(ws + L->m);
    return true;
}

// flags, then the counted entries in (b, j) order
void vm_compact(hipStream_t st, const VmRows& r) {
    hipLaunchKernelGGL(vm_flag_kernel, dim3(r.nblocks), dim3(FO_THREADS), 0, st, r);
    hipLaunchKernelGGL(fo_count_kernel<VmRows>, dim3(r.nblocks), dim3(FO_THREADS), 0, st, r);
    hipLaunchKernelGGL(fo_base_kernel<VmRows>, dim3(1), dim3(FO_THREADS), 0, st, r);
    hipLaunchKernelGGL(fo_write_index_kernel<VmRows>, dim3(r.nblocks), dim3(FO_THREADS), 0, st, r);
}

}  // namespace

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_vmf_workspace_bytes(long long rows, int C, int d) {
    VmLayout L;
    return vm_layout(rows, C, d, &L) ? L.bytes : EFFDET_EINVAL;
}

extern "C" int effdet_vmf_partition(void* stream, const float* theta, int C, int d, float* kappa, float* logz, double* logz64,
                                    double* ratio, int* clamped) {
    if (!theta || C < 1 || C > VM_MAX_CLASSES || d < 2 || d > VM_MAX_DIM || !kappa || !logz || !logz64 || !ratio || !clamped) return EFFDET_EINVAL;
    EFFDET_ENTER();
    hipLaunchKernelGGL(vm_partition_kernel, dim3((C + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), theta, C, d,
                       kappa, logz, logz64, ratio, clamped);
    return effdet_check_launch();
}

extern "C" int effdet_vmf_update(void* stream, const float* U, int B, long long P, int A, int d, const void* classes, int classes_dtype,
                                 long long classes_pitch, long long classes_stride, long long class_offset, int C, float alpha,
                                 long long rows_per_class, float* prototypes, int* valid, void* workspace, long long workspace_bytes) {
    VmRows r; VmLayout L;
    if (!vm_rows(U, B, P, A, d, classes, classes_dtype, classes_pitch, classes_stride, class_offset, C, workspace, workspace_bytes, &r, &L))
        return EFFDET_EINVAL;
    if (!vm_finite(alpha) || alpha < 0.f || alpha > 1.f || rows_per_class < 0 || !prototypes || !valid) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    r.valid = nullptr; r.need_valid = 0;
    vm_compact(st, r);
    hipLaunchKernelGGL(vm_update_kernel, dim3(C), dim3(64), 0, st, r, alpha, rows_per_class, prototypes, valid);
    return effdet_check_launch();
}

extern "C" int effdet_vmf_loss(void* stream, const float* U, int B, long long P, int A, int d, const void* classes, int classes_dtype,
                               long long classes_pitch, long long classes_stride, long long class_offset, int C, const float* prototypes,
                               const int* valid, const float* kappa, const float* logz, const double* ratio, const int* clamped,
                               float* loss, double* stats, float* dU, float* dtheta, void* workspace, long long workspace_bytes) {
    VmLoss a{}; VmLayout L;
    if (!vm_rows(U, B, P, A, d, classes, classes_dtype, classes_pitch, classes_stride, class_offset, C, workspace, workspace_bytes, &a.r, &L))
        return EFFDET_EINVAL;
    if (!prototypes || !valid || !kappa || !logz || !ratio || !clamped || !loss || !stats || !dU || !dtheta) return EFFDET_EINVAL;
    EFFDET_ENTER();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    a.r.valid = valid; a.r.need_valid = 1;
    a.h = VmHead{C, d, prototypes, reinterpret_cast<const float*>(ws + L.muT), kappa, logz, valid};
    a.ratio = ratio; a.clamped = clamped;
    a.partial = reinterpret_cast<double*>(ws + L.partial); a.nwaves = L.ngroups * VM_WAVES;
    a.loss = loss; a.dU = dU; a.dtheta = dtheta; a.stats = stats;
    a.du_elems = (long long)B * P * d;
    vm_compact(st, a.r);
    hipLaunchKernelGGL(vm_transpose_kernel, dim3((C * d + 255) / 256), dim3(256), 0, st, prototypes, reinterpret_cast<float*>(ws + L.muT), C, d);
    hipLaunchKernelGGL(vm_zero_kernel, dim3((unsigned)((a.du_elems + 255) / 256)), dim3(256), 0, st, dU, a.du_elems);
    wr_for_classes(C, [&](auto nc) {
        hipLaunchKernelGGL(vm_loss_kernel<decltype(nc)::value>, dim3(L.ngroups), dim3(VM_WAVES * 64), 0, st, a);
    });
    hipLaunchKernelGGL(vm_final_kernel, dim3(C + 3), dim3(FO_THREADS), 0, st, a);
    return effdet_check_launch();
}

extern "C" int effdet_vmf_score(void* stream, const float* U, int B, long long P, int A, int d, long long K, const long long* anchor_index,
                                const void* count, int count_is_int64, int gathered, int C, const float* prototypes, const int* valid,
                                const float* kappa, const float* logz, float* vmf, long long* vmf_class, float* vmf_cosine, float* rows,
                                void* workspace, long long workspace_bytes) {
    if (!U || B < 1 || P < 1 || A < 1 || (long long)B * P > (1ll << 31) || P * A > (1ll << 40)) return EFFDET_EINVAL;
    VmScore a{}; VmLayout L;
    if (!fo_sel(B, K, anchor_index, count, count_is_int64, P * A, &a.sel)) return EFFDET_EINVAL;
    if (!vm_layout((long long)B * K, C, d, &L) || !workspace || workspace_bytes < L.bytes) return EFFDET_EINVAL;
    if (!prototypes || !valid || !kappa || !logz || !vmf || !vmf_class || !vmf_cosine) return EFFDET_EINVAL;
    EFFDET_ENTER();
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* muT = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + L.muT);
    a.U = U; a.P = (unsigned)P; a.A = A; a.gathered = gathered ? 1 : 0;
    a.h = VmHead{C, d, prototypes, muT, kappa, logz, valid};
    a.vmf = vmf; a.cls = vmf_class; a.cosine = vmf_cosine; a.rows = rows;
    hipLaunchKernelGGL(vm_transpose_kernel, dim3((C * d + 255) / 256), dim3(256), 0, st, prototypes, muT, C, d);
    const dim3 grid((a.sel.total + VM_SCORE_ROWS - 1) / VM_SCORE_ROWS);
    wr_for_classes(C, [&](auto nc) { hipLaunchKernelGGL(vm_score_kernel<decltype(nc)::value>, grid, dim3(VM_WAVES * 64), 0, st, a); });
    return effdet_check_launch();
}

extern "C" int effdet_vmf_gather(void* stream, int dtype, int num_levels, const void* const* bases, const long long* cells,
                                 const long long* batch_strides, const long long* cell_strides, const long long* channel_strides, int F,
                                 int A, int B, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                                 float* out) {
    VmGather a{};
    if (!fo_feature_rows(dtype, num_levels, bases, cells, batch_strides, cell_strides, channel_strides, F, A, B, K, anchor_index, count,
                         count_is_int64, &a.L, &a.sel) || !out)
        return EFFDET_EINVAL;
    EFFDET_ENTER();
    a.A = A; a.F = F; a.out = out;
    hipLaunchKernelGGL(vm_gather_kernel, dim3((a.sel.total + VM_WAVES - 1) / VM_WAVES), dim3(VM_WAVES * 64), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}
