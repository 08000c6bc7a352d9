// Virtual outlier synthesis on the device (VOS, Du et al. 2022): for every class c draw S candidates
// x = mu_c + L eps, eps ~ N(0, I_F), from the class-conditional Gaussian with the tied covariance L L^T and keep the k least likely.
// The Mahalanobis distance of x is |eps|^2, so the selection works on the norms alone: the S x F candidates are never stored, and L
// is applied to the k kept rows of a class only.
//
//   random numbers   Philox4x32-10 (Salmon et al. 2011) in integer arithmetic, no state: for candidate j of class c, feature block q
//                    (features 4 q .. 4 q + 3) and draw t (int64, read on the device)
//                        counter = (j, c | q << 16, t_lo, t_hi),  key = (seed_lo, seed_hi)
//                    a word x gives u1 = (float(x >> 8) + 1) * 2^-24 in (0, 1] or u2 = float(x >> 8) * 2^-24 in [0, 1); words 0, 1 and
//                    words 2, 3 are one Box-Muller pair (u1, u2) each, float32:
//                        r = sqrtf(-2 logf(u1)),  a = fl(2 pi) * u2,  z = r * cosf(a),  r * sinf(a)
//                    so words 0 .. 3 give features 4 q .. 4 q + 3.  Every number is a function of (seed, t, c, j, d) alone.
//   norms            thread (c, j), j < S: r2 = 0, then r2 = r2 + z_d * z_d for d = 0 .. F - 1 ascending (product and sum rounded
//                    separately) -> workspace [n][S].  A lane a candidate, the feature blocks one after the other: no sum crosses a lane.
//   select           the stable LSD sort of radix_sort.h, a problem per class, on the key ~bits(r2) (r2 >= 0, so the order of the bits
//                    is the order of the floats) with the payload j: r2 descending, equal r2 by j ascending.  Four passes.
//   finish           thread (c, i), i < k: index, r2, log_density = -(r2 * 0.5) + log_const and the role of the row.
//   rows             workgroup (c, i): eps of candidate index[c][i] once more from the counter into LDS, then thread d:
//                    acc = 0, acc = acc + U[d'][d] * eps[d'] for d' = 0 .. d ascending (U = L^T, so that the threads of a wave read
//                    consecutive words), x_d = mu_c[d] + acc; zeros for a class that is not valid.  Plain float32 multiplies and adds.
//   advance          one thread: t = t + 1.
// No floating-point atomics, no host synchronisation, no allocation; every index is compared with its extent before a pointer is
// formed.  A class's results depend on (seed, t, c) and the fit alone, so any grouping of classes into calls gives the same bits.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"

namespace {

constexpr int OS_MAX_CLASSES = 1024;
constexpr int OS_MAX_FEATURES = 512;
constexpr long long OS_MAX_CANDIDATES = 1ll << 20;
constexpr long long OS_MAX_ENTRIES = 1ll << 26;                  // n * S
constexpr long long OS_MAX_ROWS = 1ll << 20;                     // n * k
constexpr int OS_THREADS = 256;

struct OsArgs {
    int F, C, n; unsigned S; int k;
    const int* ids;                                              // [n] or null: class ci
    unsigned seed_lo, seed_hi;
    long long* draw;
    const float* mu; const float* U; const float* log_const; const signed char* valid;
    float* r2ws;                                                 // [n][S]
    const unsigned *skey, *sidx;                                 // [n][S]: the sorted keys and candidates
    float* rows; int* index; float* r2; float* logd; signed char* roles;
};

DEV void os_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

DEV void os_pair(unsigned x, unsigned y, float& z0, float& z1) {
    const float u1 = ((float)(x >> 8) + 1.0f) * 5.9604644775390625e-8f, u2 = (float)(y >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1)), a = 6.2831853071795864769f * u2;
    z0 = r * cosf(a); z1 = r * sinf(a);
}

// the four normals of feature block q of candidate j of class c at draw t
DEV void os_normals(const OsArgs& a, unsigned c, unsigned j, unsigned q, unsigned t_lo, unsigned t_hi, float (&z)[4]) {
    unsigned w[4];
    os_philox(j, c | (q << 16), t_lo, t_hi, a.seed_lo, a.seed_hi, w);
    os_pair(w[0], w[1], z[0], z[1]);
    os_pair(w[2], w[3], z[2], z[3]);
}

DEV int os_class(const OsArgs& a, unsigned ci) { return a.ids ? a.ids[ci] : (int)ci; }

__global__ __launch_bounds__(OS_THREADS) void os_norms_kernel(OsArgs a) {
    const unsigned ci = blockIdx.y, j = (unsigned)blockIdx.x * OS_THREADS + threadIdx.x;
    if (j >= a.S) return;
    const unsigned c = (unsigned)os_class(a, ci) & 0xFFFFu;
    const unsigned long long t = (unsigned long long)a.draw[0];
    const unsigned t_lo = (unsigned)t, t_hi = (unsigned)(t >> 32);
    float r2 = 0.f;
    const unsigned nq = (unsigned)a.F >> 2;
#pragma unroll 2
    for (unsigned q = 0; q < nq; ++q) {
        float z[4];
        os_normals(a, c, j, q, t_lo, t_hi, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) r2 = r2 + z[e] * z[e];
    }
    a.r2ws[(unsigned long long)ci * a.S + j] = r2;
}

// ---- select: the pass descriptor of radix_sort.h -------------------------------------------------------------------------------
struct OsItem { unsigned key; unsigned idx; };
struct OsSort {
    typedef unsigned Key;
    typedef OsItem Item;
    const float* r2;                                             // first pass: the keys come from here, the payload is the position
    const unsigned *ink, *ini; unsigned *outk, *outi;            // [n][S]
    unsigned* hist; unsigned* totals;
    unsigned S, tiles;
    int shift, first;
};
DEV RsProblem rs_problem(const OsSort& p, unsigned y) {
    return RsProblem{p.S, p.hist + (unsigned long long)y * 256u * p.tiles, p.totals + y * 256u, p.tiles};
}
DEV unsigned rs_key(const OsSort& p, unsigned y, unsigned i) {
    const unsigned long long at = (unsigned long long)y * p.S + i;
    return p.first ? ~(unsigned)__float_as_int(p.r2[at]) : p.ink[at];
}
DEV OsItem rs_load(const OsSort& p, unsigned y, unsigned i) {
    return OsItem{rs_key(p, y, i), p.first ? i : p.ini[(unsigned long long)y * p.S + i]};
}
DEV void rs_store(const OsSort& p, unsigned y, unsigned pos, const OsItem& e) {
    const unsigned long long at = (unsigned long long)y * p.S + pos;
    p.outk[at] = e.key; p.outi[at] = e.idx;
}

__global__ __launch_bounds__(OS_THREADS) void os_finish_kernel(OsArgs a) {
    const unsigned e = (unsigned)blockIdx.x * OS_THREADS + threadIdx.x;
    if (e >= (unsigned)a.n * (unsigned)a.k) return;
    const unsigned ci = e / (unsigned)a.k, i = e - ci * (unsigned)a.k;
    const unsigned long long at = (unsigned long long)ci * a.S + i;         // i < k <= S
    const int c = os_class(a, ci);
    const bool ok = c >= 0 && c < a.C && a.valid[c] != 0;
    const float r2 = __int_as_float((int)~a.skey[at]);
    a.index[e] = (int)a.sidx[at];
    a.r2[e] = r2;
    a.logd[e] = -(r2 * 0.5f) + a.log_const[0];
    a.roles[e] = ok ? (signed char)0 : (signed char)-1;
}

__global__ __launch_bounds__(OS_THREADS) void os_rows_kernel(OsArgs a) {
    __shared__ float eps[OS_MAX_FEATURES];
    const unsigned e = blockIdx.x;                               // < n * k
    const unsigned ci = e / (unsigned)a.k;
    const int tid = threadIdx.x, F = a.F;
    const int c = os_class(a, ci);
    const bool ok = c >= 0 && c < a.C && a.valid[c] != 0;        // the same for the whole workgroup
    float* out = a.rows + (unsigned long long)e * F;
    if (!ok) {
        for (int d = tid; d < F; d += OS_THREADS) out[d] = 0.f;
        return;
    }
    const unsigned j = (unsigned)a.index[e];
    const unsigned long long t = (unsigned long long)a.draw[0];
    for (int q = tid; q < (F >> 2); q += OS_THREADS) {
        float z[4];
        os_normals(a, (unsigned)c, j, (unsigned)q, (unsigned)t, (unsigned)(t >> 32), z);
#pragma unroll
        for (int s = 0; s < 4; ++s) eps[4 * q + s] = z[s];
    }
    __syncthreads();
    const float* mu = a.mu + (long long)c * F;
    for (int d = tid; d < F; d += OS_THREADS) {
        float acc = 0.f;
        for (int dp = 0; dp <= d; ++dp) acc = acc + a.U[(long long)dp * F + d] * eps[dp];
        out[d] = mu[d] + acc;
    }
}

__global__ void os_advance_kernel(long long* draw) {
    if (blockIdx.x == 0 && threadIdx.x == 0) draw[0] = draw[0] + 1;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct OsLayout { long long r2, ka, ia, kb, ib, hist, totals, bytes; unsigned tiles; };

bool os_layout(int n, long long S, OsLayout* L) {
    if (n < 1 || n > OS_MAX_CLASSES || S < 1 || S > OS_MAX_CANDIDATES || (long long)n * S > OS_MAX_ENTRIES) return false;
    const long long e = (long long)n * S * 4;
    L->tiles = (unsigned)((S + RS_TILE - 1) / RS_TILE);
    FoCarve ws;
    L->r2 = ws.take(e);
    L->ka = ws.take(e);
    L->ia = ws.take(e);
    L->kb = ws.take(e);
    L->ib = ws.take(e);
    L->hist = ws.take((long long)n * 256 * L->tiles * 4);
    L->totals = ws.take((long long)n * 256 * 4);
    L->bytes = ws.at;
    return true;
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_outlier_synth_workspace_bytes(int n, long long S) {
    OsLayout L;
    return os_layout(n, S, &L) ? L.bytes : EFFDET_EINVAL;
}

extern "C" int effdet_outlier_synth(void* stream, int F, int C, int n, const int* class_ids, long long S, int k,
                                    unsigned long long seed, long long* draw, int advance, const float* mu, const float* U,
                                    const float* log_const, const signed char* valid, float* rows, int* index, float* r2,
                                    float* log_density, signed char* roles, void* workspace, long long workspace_bytes) {
    if (F < 4 || F > OS_MAX_FEATURES || (F & 3) || C < 1 || C > OS_MAX_CLASSES) return EFFDET_EINVAL;
    OsLayout L;
    if (!os_layout(n, S, &L)) return EFFDET_EINVAL;
    if (k < 1 || k > S || (long long)n * k > OS_MAX_ROWS) return EFFDET_EINVAL;
    if (!draw || !mu || !U || !log_const || !valid || !rows || !index || !r2 || !log_density || !roles) return EFFDET_EINVAL;
    if (!workspace || workspace_bytes < L.bytes) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    char* ws = reinterpret_cast<char*>(workspace);
    const auto u32 = [&](long long at) { return reinterpret_cast<unsigned*>(ws + at); };
    OsArgs a{};
    a.F = F; a.C = C; a.n = n; a.S = (unsigned)S; a.k = k;
    a.ids = class_ids;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
    a.draw = draw;
    a.mu = mu; a.U = U; a.log_const = log_const; a.valid = valid;
    a.r2ws = reinterpret_cast<float*>(ws + L.r2);
    a.skey = u32(L.kb); a.sidx = u32(L.ib);                      // four passes: r2 -> a -> b -> a -> b
    a.rows = rows; a.index = index; a.r2 = r2; a.logd = log_density; a.roles = roles;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(os_norms_kernel, dim3((a.S + OS_THREADS - 1) / OS_THREADS, n), dim3(OS_THREADS), 0, st, a);
    OsSort p{};
    p.r2 = a.r2ws; p.hist = u32(L.hist); p.totals = u32(L.totals); p.S = a.S; p.tiles = L.tiles;
    for (int pass = 0; pass < 4; ++pass) {
        const bool to_a = (pass & 1) == 0;
        p.shift = 8 * pass; p.first = pass == 0;
        p.ink = u32(to_a ? L.kb : L.ka); p.ini = u32(to_a ? L.ib : L.ia);
        p.outk = u32(to_a ? L.ka : L.kb); p.outi = u32(to_a ? L.ia : L.ib);
        rs_sort_pass(st, p, L.tiles, (unsigned)n);
    }
    const unsigned nrows = (unsigned)n * (unsigned)k;
    hipLaunchKernelGGL(os_finish_kernel, dim3((nrows + OS_THREADS - 1) / OS_THREADS), dim3(OS_THREADS), 0, st, a);
    hipLaunchKernelGGL(os_rows_kernel, dim3(nrows), dim3(OS_THREADS), 0, st, a);
    if (advance) hipLaunchKernelGGL(os_advance_kernel, dim3(1), dim3(1), 0, st, draw);
    return effdet_check_launch();
}
