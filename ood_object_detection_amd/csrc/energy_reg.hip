// Energy-margin OOD training losses on the device, forward and backward: the energy-bounded hinge (Liu et al. 2020) and the
// logistic uncertainty loss of VOS (Du et al. 2022) over rows of C class logits with a role per row.
//
//   per row, float32, z the C logits (bfloat16 widened exactly), role 1 = in-distribution, 0 = outlier, anything else: not counted
//     logsumexp   mz = max z, m = mz / T, s = sum_k exp(z_k / T - m), E = -(T * (m + log s)),  dE/dz_k = -(exp(z_k / T - m) / s)
//     joint       E = -sum_k (max(z_k, 0) + log1p(exp(-|z_k|))),                                dE/dz_k = -(1 / (1 + exp(-z_k)))
//     an outlier row counts only when mz >= min_max_logit (a row that holds a NaN has a NaN maximum and does not pass)
//     hinge       in: d = E - m_in, out: d = m_out - E;  h = d < 0 ? 0 : d;  l = h * h,  dl/dE = +-(2 * h)
//     logistic    sv = w * (-E) + b;  in: l = softplus(-sv), dl/dsv = -sigmoid(-sv);  out: l = softplus(sv), dl/dsv = sigmoid(sv);
//                 dl/dE = dl/dsv * (-w)
//     E, dE/dz, dl/dE and with them grad z are float32 in that order.  The terms of the float64 sums over rows - l and dl/dsv - are
//     evaluated in float64 by the kernel that adds them, a thread a row: the hinge's l = h * h from the float32 h (so that it is
//     positive exactly where grad z is not zero); the logistic terms from the float32 m and s of the log-sum-exp (E once more as
//     -(T * (m + log s)) in float64) or from the float32 joint energy, with w, b widened - a log, an exp and a log1p a row, so that
//     a sum keeps the rounding of the float32 sum over the classes and nothing after it
//   loss = c_in * sum_in l + c_out * sum_out l with c_side = weight_side / max(n_side, 1) in float64;
//   grad z_k = (float(c_side) * dl/dE) * dE/dz_k;  grad w = sum_side c_side * sum dl/dsv * (-E),  grad b = sum_side c_side * sum dl/dsv
//
//   rows     16 rows per workgroup of four waves.  A wave takes four rows one after the other: lane t holds classes t, t + 64, ...
//            in registers, every sum runs over a lane's classes ascending and then over the lanes by the xor tree 32 .. 1.  A row
//            whose role does not count is not read.  Per row the kernel leaves its side, E, m, s and dl/dE.
//   partial  workgroup k forms and adds the float64 terms of rows [2048 k, 2048 (k + 1)): a thread its eight rows ascending, then the
//            tree of compact.h.
//   final    one workgroup adds the partials (a thread every 256th, ascending, then the tree), writes the loss, the statistics,
//            grad_phi and the two float32 row coefficients.  The counts never leave the device.
//   grad     the rows layout again: a row that does not count, or whose coefficient times dl/dE is zero, gets zeros without its
//            logits being read; the others are read a second time.
// No floating-point atomics; the order of every sum follows from the number of rows alone.  Every row index is compared with its
// extent before a pointer is formed, every store index before the store; no call synchronises with the host or allocates.
#include "common.h"
#include "feature_rows.h"
#include "wave_rows.h"

namespace {

constexpr int ER_MAX_CLASSES = 1024;
constexpr int ER_ROWS = 16;                                      // rows of a workgroup
constexpr int ER_WAVES = 4;
constexpr int ER_TERMS = 12;                                     // n, sum l, sum E, active, sum dl/dsv * (-E), sum dl/dsv; per side
constexpr int ER_HINGE = 0, ER_LOGISTIC = 1, ER_LSE = 0, ER_JOINT = 1;

struct ErArgs {
    const void* z; int bf16, C; unsigned total;                 // contiguous [total][C]
    const signed char* role;                                    // [total]
    int form, kind; float T, m_in, m_out; double w_in, w_out;
    int use_min; float min_max;
    const float* phi;                                           // (w, b); null for the hinge
    signed char* side;                                          // workspace, per row: 0 not counted, 1 in, 2 out
    float *E, *m, *s, *dE;
    double* partial; unsigned nblocks; float* coef;
    float* loss; double* stats; float* energy; void* grad; float* grad_phi;
};

DEV float er_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

DEV const char* er_rowp(const ErArgs& a, unsigned i) {
    return reinterpret_cast<const char*>(a.z) + (long long)i * a.C * (a.bf16 ? 2 : 4);
}
// float32 -> bfloat16 bits, round to nearest even (a NaN becomes the quiet NaN 0x7FC0, as torch's conversion writes it)
DEV unsigned short er_bf16(float v) {
    const unsigned b = (unsigned)__float_as_int(v);
    if (v != v) return (unsigned short)0x7FC0u;
    return (unsigned short)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

template <int NC>
__global__ __launch_bounds__(ER_WAVES * 64) void er_rows_kernel(ErArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const unsigned i = (unsigned)blockIdx.x * ER_ROWS + wave * 4 + rr;      // the same for the whole wave
        if (i >= a.total) continue;
        const int role = a.role[i];
        int side = role == 1 ? 1 : (role == 0 ? 2 : 0);
        float E = 0.f, m = 0.f, s = 0.f, dE = 0.f;
        if (side) {
            float z[NC];
            wr_load<NC>(er_rowp(a, i), C, a.bf16, lane, z);
            float mz = -__builtin_inff();                       // the maximum and the NaN test in one pass over the registers
            bool bad = false;
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (lane + 64 * k < C) { mz = fmaxf(mz, z[k]); bad = bad || z[k] != z[k]; }
            mz = wave_reduce_max(mz);
            const bool nan = __ballot(bad) != 0ull;
            if (side == 2 && a.use_min && (nan || !(mz >= a.min_max))) side = 0;
            if (side) {                                         // (uniform over the wave)
                if (a.kind == ER_LSE) {
                    wr_lse<NC>(z, C, a.T, mz, lane, &m, &s);
                    const float lse = m + logf(s);
                    E = -(a.T * lse);
                } else {
                    float t = 0.f;
#pragma unroll
                    for (int k = 0; k < NC; ++k) t += lane + 64 * k < C ? wr_softplus(z[k]) : 0.f;
                    E = -wave_reduce_sum(t);
                }
                if (a.form == ER_HINGE) {
                    const float d = side == 1 ? E - a.m_in : a.m_out - E;
                    const float h = d < 0.f ? 0.f : d;          // (a NaN stays one)
                    dE = side == 1 ? 2.f * h : -(2.f * h);
                } else {
                    const float w = a.phi[0], b = a.phi[1];
                    const float sv = w * (-E) + b;
                    const float ds = side == 1 ? -er_sigmoid(-sv) : er_sigmoid(sv);
                    dE = ds * (-w);
                }
            }
        }
        if (lane == 0) {
            a.side[i] = (signed char)side;
            if (side) { a.E[i] = E; a.m[i] = m; a.s[i] = s; a.dE[i] = dE; }
            if (a.energy) a.energy[i] = side ? E : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void er_partial_kernel(ErArgs a) {
    __shared__ double sh[FO_THREADS];
    const int tid = threadIdx.x;
    double acc[ER_TERMS];
#pragma unroll
    for (int q = 0; q < ER_TERMS; ++q) acc[q] = 0.0;
    float w = 0.f, b = 0.f;
    if (a.form == ER_LOGISTIC) { w = a.phi[0]; b = a.phi[1]; }
    for (int r = 0; r < FO_ITEMS; ++r) {
        const unsigned i = (unsigned)blockIdx.x * FO_TILE + r * FO_THREADS + tid;
        if (i >= a.total) continue;
        const int side = a.side[i];
        if (side != 1 && side != 2) continue;
        const int o = side - 1;
        const float E = a.E[i];
        double Ed = (double)E, l, dsv = 0.0, active = 0.0;
        if (a.form == ER_HINGE) {                               // d, h: the float32 operations of the rows kernel, so that the loss
            const float d = side == 1 ? E - a.m_in : a.m_out - E;       // is positive exactly where grad_logits is not zero
            const float h = d < 0.f ? 0.f : d;                  // (a NaN stays one)
            l = (double)h * (double)h;
            active = h > 0.f ? 1.0 : 0.0;
        } else {
            // the energy the logistic terms read: for the log-sum-exp its last three operations (log, + m, T *) once more in float64
            // from the float32 m and s, so that l keeps the rounding of the sum of exponentials and not that of the energy's last place
            if (a.kind == ER_LSE) Ed = -((double)a.T * ((double)a.m[i] + log((double)a.s[i])));
            const double sv = (double)w * -Ed + (double)b, x = side == 1 ? -sv : sv;
            const double e = exp(-fabs(x)), sg = (x < 0.0 ? e : 1.0) / (1.0 + e);      // sigmoid(x)
            l = (x < 0.0 ? 0.0 : x) + log1p(e);                                         // softplus(x); a NaN stays one
            dsv = side == 1 ? -sg : sg;
        }
        acc[o] += 1.0;                                          // counts <= 2^27: exact
        acc[2 + o] += l;
        acc[4 + o] += (double)E;
        acc[6 + o] += active;
        acc[8 + o] += dsv * -Ed;
        acc[10 + o] += dsv;
    }
    for (int q = 0; q < ER_TERMS; ++q) {
        const double t = fo_block_sum<double>(acc[q], sh, tid);
        if (tid == 0) a.partial[(long long)blockIdx.x * ER_TERMS + q] = t;
    }
}

__global__ __launch_bounds__(256) void er_final_kernel(ErArgs a) {
    __shared__ double sh[FO_THREADS];
    __shared__ double tot[ER_TERMS];
    const int tid = threadIdx.x;
    for (int q = 0; q < ER_TERMS; ++q) {
        double t = 0.0;
        for (unsigned k = tid; k < a.nblocks; k += FO_THREADS) t += a.partial[(long long)k * ER_TERMS + q];
        t = fo_block_sum<double>(t, sh, tid);
        if (tid == 0) tot[q] = t;
    }
    if (tid != 0) return;
    const double n_in = tot[0], n_out = tot[1];
    const double d_in = n_in < 1.0 ? 1.0 : n_in, d_out = n_out < 1.0 ? 1.0 : n_out;
    const double c_in = a.w_in / d_in, c_out = a.w_out / d_out;
    a.loss[0] = (float)(c_in * tot[2] + c_out * tot[3]);
    a.stats[0] = n_in; a.stats[1] = n_out;
    a.stats[2] = tot[2] / d_in; a.stats[3] = tot[3] / d_out;
    a.stats[4] = tot[4] / d_in; a.stats[5] = tot[5] / d_out;
    a.stats[6] = tot[6]; a.stats[7] = tot[7];
    a.grad_phi[0] = (float)(c_in * tot[8] + c_out * tot[9]);
    a.grad_phi[1] = (float)(c_in * tot[10] + c_out * tot[11]);
    a.coef[0] = (float)c_in; a.coef[1] = (float)c_out;
}

template <int NC>
__global__ __launch_bounds__(ER_WAVES * 64) void er_grad_kernel(ErArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const unsigned i = (unsigned)blockIdx.x * ER_ROWS + wave * 4 + rr;      // the same for the whole wave
        if (i >= a.total) continue;
        const int side = a.side[i];
        float g = 0.f;
        if (side == 1 || side == 2) g = a.coef[side - 1] * a.dE[i];
        float out[NC];
        if (g == 0.f) {                                         // not counted, or a hinge that is not active (a NaN is not zero)
#pragma unroll
            for (int k = 0; k < NC; ++k) out[k] = 0.f;
        } else {
            float z[NC];
            wr_load<NC>(er_rowp(a, i), C, a.bf16, lane, z);
            if (a.kind == ER_LSE) {
                const float m = a.m[i], s = a.s[i];
#pragma unroll
                for (int k = 0; k < NC; ++k) { const float p = expf(z[k] / a.T - m) / s; out[k] = g * -p; }
            } else {
#pragma unroll
                for (int k = 0; k < NC; ++k) out[k] = g * -er_sigmoid(z[k]);
            }
        }
        const long long base = (long long)i * C;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                if (a.bf16) reinterpret_cast<unsigned short*>(a.grad)[base + c] = er_bf16(out[k]);
                else reinterpret_cast<float*>(a.grad)[base + c] = out[k];
            }
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct ErLayout { long long side, E, m, s, dE, partial, coef, bytes; unsigned nblocks; };

bool er_layout(long long rows, ErLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS) return false;
    L->nblocks = (unsigned)((rows + FO_TILE - 1) / FO_TILE);
    FoCarve ws;
    L->side = ws.take(rows);
    L->E = ws.take(rows * 4);
    L->m = ws.take(rows * 4);
    L->s = ws.take(rows * 4);
    L->dE = ws.take(rows * 4);
    L->partial = ws.take((long long)L->nblocks * ER_TERMS * 8);
    L->coef = ws.take(256);
    L->bytes = ws.at;
    return true;
}

bool er_finite(float v) { return v - v == 0.f; }

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_energy_reg_workspace_bytes(long long rows) {
    ErLayout L;
    return er_layout(rows, &L) ? L.bytes : EFFDET_EINVAL;
}

extern "C" int effdet_energy_reg(void* stream, int dtype, const void* logits, const signed char* role, int B, long long N, int C,
                                 int form, int energy_kind, float temperature, float margin_in, float margin_out, float weight_in,
                                 float weight_out, int use_min, float min_max_logit, const float* phi, float* loss, double* stats,
                                 float* energy, void* grad_logits, float* grad_phi, void* workspace, long long workspace_bytes) {
    if ((dtype != EFFDET_F32 && dtype != EFFDET_BF16) || !logits || !role || B < 1 || N < 1 || N > FO_MAX_ROWS) return EFFDET_EINVAL;
    if (C < 1 || C > ER_MAX_CLASSES) return EFFDET_EINVAL;
    ErLayout L;
    if (!er_layout((long long)B * N, &L)) return EFFDET_EINVAL;
    if ((form != ER_HINGE && form != ER_LOGISTIC) || (energy_kind != ER_LSE && energy_kind != ER_JOINT)) return EFFDET_EINVAL;
    if (!(temperature > 0.f) || !er_finite(temperature) || (energy_kind == ER_JOINT && temperature != 1.f)) return EFFDET_EINVAL;
    if (form == ER_HINGE && (!er_finite(margin_in) || !er_finite(margin_out))) return EFFDET_EINVAL;
    if (form == ER_LOGISTIC && !phi) return EFFDET_EINVAL;
    if (!er_finite(weight_in) || !er_finite(weight_out) || (use_min && !(min_max_logit == min_max_logit))) return EFFDET_EINVAL;
    if (!loss || !stats || !grad_phi || !workspace || workspace_bytes < L.bytes) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    ErArgs a{};
    a.z = logits; a.bf16 = dtype == EFFDET_BF16; a.C = C; a.total = (unsigned)((long long)B * N);
    a.role = role;
    a.form = form; a.kind = energy_kind; a.T = temperature; a.m_in = margin_in; a.m_out = margin_out;
    a.w_in = (double)weight_in; a.w_out = (double)weight_out;
    a.use_min = use_min ? 1 : 0; a.min_max = min_max_logit;
    a.phi = form == ER_LOGISTIC ? phi : nullptr;
    char* ws = reinterpret_cast<char*>(workspace);
    a.side = reinterpret_cast<signed char*>(ws + L.side);
    a.E = reinterpret_cast<float*>(ws + L.E); a.m = reinterpret_cast<float*>(ws + L.m); a.s = reinterpret_cast<float*>(ws + L.s);
    a.dE = reinterpret_cast<float*>(ws + L.dE);
    a.partial = reinterpret_cast<double*>(ws + L.partial); a.nblocks = L.nblocks; a.coef = reinterpret_cast<float*>(ws + L.coef);
    a.loss = loss; a.stats = stats; a.energy = energy; a.grad = grad_logits; a.grad_phi = grad_phi;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((a.total + ER_ROWS - 1) / ER_ROWS), block(ER_WAVES * 64);
    wr_for_classes(C, [&](auto nc) { hipLaunchKernelGGL(er_rows_kernel<decltype(nc)::value>, grid, block, 0, st, a); });
    hipLaunchKernelGGL(er_partial_kernel, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(er_final_kernel, dim3(1), dim3(FO_THREADS), 0, st, a);
    if (grad_logits) wr_for_classes(C, [&](auto nc) { hipLaunchKernelGGL(er_grad_kernel<decltype(nc)::value>, grid, block, 0, st, a); });
    return effdet_check_launch();
}
