// Detection calibration on the device: reliability tables of the detection score under the PASCAL matching of
// eval_scale.hip (D-ECE, MCE, ACE, classwise ECE, LaECE, Brier, NLL are host glue over them), and a post-hoc monotone calibrator
// p' = sigmoid(a logit(p~) + b) fitted by a damped Newton iteration that never leaves the device.  Compiled with
// -ffp-contract=off: the IoU rounds like eval_scale.hip's, every float64 term below is one operation, one rounding each.
//
// Definitions (restated in tests/_calibration_ref.py).
//   match    es_match_kernel of eval_scale.hip, the same flag words and counters (bit t true positive at threshold t, bit 16 + t
//            ignored there: the candidate is `difficult`, bit 31 dropped), and per slot the float32 IoU with the candidate box: the
//            box of the detection's class with the largest IoU, the lowest index on ties; 0 where the class has no box or the slot
//            is dropped.  The candidate does not depend on the threshold.
//   append   a slot is kept iff it lies below the count, is not dropped and score >= score_threshold (after the matching: a
//            low-score detection still takes its box).  (score, class, flag word, IoU) go to the capacity-sized buffers at the
//            device cursor, ev_append of eval_sorted.h; overflow and NaN scores are counted there.
//   sort     by (class, score descending, arrival order on equal scores) with the flag word and the IoU as payload; then the
//            sorted entries once more by score alone (the `pooled` scope: equal scores in (class, arrival) order).
//   scopes   s = 0 .. C-1: the entries of class s; s = C: pooled.  A scope with m kept entries is one contiguous range of a sorted
//            array; position 0 is its largest score.
//   bins     width: k = min(K - 1, max(0, (int)(p * (float)K))), one float32 product; the score order makes every bin a
//            contiguous range (bin K - 1 first).  mass: bin k = positions [floor(k m / K), floor((k + 1) m / K)), 64-bit integers;
//            entries ignored at t keep their position and add nothing.
//   tables   per (t, s, scheme, k) over the bin's entries not ignored at t: n, tp (int64), sum_p = the sum of (double)p, sum_iou =
//            the sum of (double)IoU over the true positives.  Per (t, s): brier = the sum of (p - y)^2 with y = tp, nll = minus the
//            sum of log(y ? p~ : 1 - p~) with p~ = p clamped to [2^-24, 1 - 2^-24], out_of_range = scores outside [0, 1] (NaN
//            scores never arrive), entries = m.
//   order    every float64 sum of a range [lo, hi): thread j of 256 adds the entries lo + j, lo + j + 256, ... in ascending order
//            from 0.0; the 256 thread sums are then added by ev_block_sum of eval_sorted.h (the xor butterfly 32, 16, .. 1 inside
//            a wave, then the four waves in ascending order).  The order depends on the sorted positions alone: the same images
//            give the same bits from run to run and for every split into batches.  No floating-point atomics.
//   fit      over the UNSORTED entries i < live count that are not ignored at the chosen threshold: x = log(p~ / (1 - p~)),
//            z = a x + b, s = sigmoid(z), target y = tp (target 'tp') or tp ? IoU : 0 (target 'iou'); NLL = the sum of
//            log(1 + exp(z)) - y z, gradient (sum (s - y) x, sum (s - y)), Hessian (sum w x x, sum w x, sum w), w = s (1 - s), all in
//            float64.  Launch 1: workgroup g sums the entries [2048 g, 2048 (g + 1)) at the trial point (thread j: 2048 g + j,
//            + 256, ... ascending; then ev_block_sum) into partials[g].  Launch 2: one workgroup; thread q adds partial sum q of the
//            live groups in ascending g, thread 0 then advances the state block: the first evaluation is accepted when finite; a
//            later trial is accepted iff its NLL is finite and <= NLL_accepted (1 + 2^-40), else the step halves (a step below
//            2^-60 gives up).  At an accepted point the Newton direction d = -H^-1 g (temperature: -g_a / H_aa, b stays 0) is
//            taken; a Hessian that is not positive definite or a direction that is not finite gives up; max(|d_a|, |d_b|) <=
//            2^-40 max(1, |a|, |b|) is convergence.  Giving up and convergence freeze the state: later launches exit at once.
//   apply    det_out = det_in with column 4 of the slots below the count replaced by float32(sigmoid(a logit(p~) + b)), computed
//            in float64 with (a, b) read from the state block on the device; a NaN score stays NaN.
//
// Launch boundaries are the only synchronisation between workgroups.  Every loop has a trip count known at its entry, every store
// index is compared with the live count or the capacity; the live count is read from the device cursor, nothing is read back: the
// unit is capturable.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"
#include "eval_match.h"
#include "eval_sorted.h"

namespace {

constexpr int CA_THREADS = EV_THREADS;
constexpr int CA_MAX_T = 16, CA_MAX_K = 64;
constexpr long long CA_MAX_CELLS = 1ll << 20;                     // T (C + 1) K: the result block stays below 72 MiB
constexpr unsigned CA_INVALID = 0x80000000u;
constexpr int CA_RESULT_HEAD = 8;                                 // 8-byte words before the tables
constexpr int CA_PARTS = 3;                                       // width bins, mass bins, the scope's totals
constexpr int CA_FIT_CHUNK = EV_AP_CHUNK;                         // entries of one fit workgroup
constexpr int CA_FIT_SUMS = 8;                                    // NLL, g_a, g_b, H_aa, H_ab, H_bb, entries, 0
constexpr int CA_FIT_STATE = 16;                                  // doubles of the state block
// the state block: accepted a, b and NLL; trial a, b; step scale; direction a, b; first NLL; evaluations; halvings; converged;
// frozen; an accepted point exists; entries used; 0
enum { CA_A, CA_B, CA_NLL, CA_TA, CA_TB, CA_LAM, CA_DA, CA_DB, CA_NLL0, CA_ITER, CA_HALV, CA_CONV, CA_FROZEN, CA_HAVE, CA_COUNT };

DEV float ca_score(u64 key) { return __uint_as_float(fo_unkey(~(unsigned)(key & 0xFFFFFFFFull))); }
// the width bin of score p; equal to min(K - 1, max(0, (int)(p * (float)K))) wherever that cast is defined
DEV int ca_bin(float p, int K) {
    const float q = p * (float)K;
    return q >= (float)K ? K - 1 : (q > 0.f ? (int)q : 0);
}
DEV double ca_clamp(double p) { return p < 0x1p-24 ? 0x1p-24 : (p > 1.0 - 0x1p-24 ? 1.0 - 0x1p-24 : p); }
DEV double ca_logit(double p) { const double c = ca_clamp(p); return log(c / (1.0 - c)); }
DEV double ca_sigmoid(double z) { const double e = exp(-fabs(z)); return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e); }
DEV bool ca_finite(double v) { return v - v == 0.0; }

// ---- matching: es_match_kernel of eval_scale.hip, and the candidate's IoU per slot ------------------------------------------------
struct CaMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls; const unsigned char* gt_difficult;
    int B, max_det, M, C, T; float thr[CA_MAX_T]; float score_thr;
    unsigned* flags; float* iou; int* kept; int* gt_count; int* gt_imgs; int* correct;
};

__global__ __launch_bounds__(CA_THREADS) void ca_match_kernel(CaMatch p) {
    extern __shared__ int ca_lds[];
    int* seen = ca_lds;                              // [C] class already had its top-scoring detection
    int* taken = ca_lds + p.C;                       // [M] bit t: taken at threshold t
    int* gcls = taken + p.M;                         // [M] 0-based class or -1
    int* gdif = gcls + p.M;                          // [M]
    float* red_v = reinterpret_cast<float*>(gdif + p.M);    // [4]
    int* red_i = reinterpret_cast<int*>(red_v + 4);          // [4]
    const int b = blockIdx.x, tid = threadIdx.x;
    em_stage_gt(p.gt_cls, p.gt_difficult, b, p.M, p.C, seen, taken, gcls, gdif, p.gt_count, p.gt_imgs);
    const int n = min(p.det_count[b], p.max_det);
    int kept = 0, nans = 0;                          // thread 0's
    for (int i = 0; i < p.max_det; ++i) {
        const long long slot = (long long)b * p.max_det + i;
        if (i >= n) { if (tid == 0) { p.flags[slot] = CA_INVALID; p.iou[slot] = 0.f; } continue; }
        const float* d = p.det + slot * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4];
        const int c = (int)d[5] - 1;
        if (score != score) ++nans;
        if (!(y1 < y2 && x1 < x2) || c < 0 || c >= p.C || score != score) {     // uniform
            if (tid == 0) { p.flags[slot] = CA_INVALID; p.iou[slot] = 0.f; }
            continue;
        }
        float best;
        const int bj = em_best_box(em_det(x1, y1, x2, y2), c, p.gt_boxes, gcls, b, p.M, red_v, red_i, &best);
        if (tid == 0) {
            const bool has_gt = bj != EM_NO_BOX;
            unsigned word = 0, reach = 0;            // reach: thresholds the candidate's IoU reaches
            if (has_gt) {
                for (int t = 0; t < p.T; ++t) reach |= (best >= p.thr[t] ? 1u : 0u) << t;
                if (gdif[bj]) {
                    word = reach << 16;
                } else {
                    word = reach & ~(unsigned)taken[bj];
                    taken[bj] |= (int)reach;
                }
            }
            p.flags[slot] = word;
            p.iou[slot] = (has_gt && !(word & CA_INVALID)) ? best : 0.f;     // T = 16, ignored at all 16 thresholds: bit 31, dropped
            if (!(word & CA_INVALID) && score >= p.score_thr) ++kept;     // what ev_keep below keeps
            if (!seen[c]) {                                                          // top-scoring detection of class c
                seen[c] = 1;
                for (int t = 0; t < p.T; ++t)
                    if ((reach >> t) & 1u) atomicAdd(p.correct + (long long)t * p.C + c, 1);
            }
        }
        __syncthreads();
    }
    if (tid == 0) { p.kept[b] = kept; p.kept[p.B + b] = nans; }
}

// ---- append: the flag word and the IoU travel with (score, class) ---------------------------------------------------------------------
struct CaAppend : EvAppend { const unsigned* flags; const float* iou; unsigned* out_flags; float* out_iou; float score_thr; };
DEV bool ev_keep(const CaAppend& a, long long slot, unsigned* word) {
    *word = a.flags[slot];
    return !(*word & CA_INVALID) && a.det[slot * 6 + 4] >= a.score_thr;
}
DEV void ev_store(const CaAppend& a, long long slot, unsigned p, unsigned word) { a.out_flags[p] = word; a.out_iou[p] = a.iou[slot]; }

// ---- sort: by (class, score descending), flag word and IoU bits as payload; then the sorted entries again by score alone ----------
struct CaItem { u64 key; unsigned val, iou; };
struct CaSort : EvSort {
    typedef CaItem Item;
    const unsigned* flags; const unsigned* iou;                           // the first pass reads these
    const unsigned* src_w; unsigned* dst_w;
};
DEV u64 rs_key(const CaSort& s, unsigned, unsigned i) {
    return ev_key(s, i, [&s](unsigned k) { return !(s.flags[k] & CA_INVALID); });
}
DEV CaItem rs_load(const CaSort& s, unsigned, unsigned i) {
    return CaItem{rs_key(s, 0, i), s.first ? s.flags[i] : s.src_v[i], s.first ? s.iou[i] : s.src_w[i]};
}
DEV void rs_store(const CaSort& s, unsigned, unsigned p, const CaItem& e) { s.dst_k[p] = e.key; s.dst_v[p] = e.val; s.dst_w[p] = e.iou; }

// pk, pv, pw: the class-sorted keys, flag words and IoU bits.  The key keeps the score part; its class becomes 0, or 1 for an
// entry that is not valid: the stable sort leaves equal scores in (class, arrival) order.
struct CaPoolSort : EvSort {
    typedef CaItem Item;
    const u64* pk; const unsigned* pv; const unsigned* pw; const unsigned* src_w; unsigned* dst_w; int num_classes;
};
DEV u64 rs_key(const CaPoolSort& s, unsigned, unsigned i) {
    if (!s.first) return s.src_k[i];
    const u64 k = s.pk[i];
    return ((u64)((unsigned)(k >> 32) < (unsigned)s.num_classes ? 0u : 1u) << 32) | (k & 0xFFFFFFFFull);
}
DEV CaItem rs_load(const CaPoolSort& s, unsigned, unsigned i) {
    return CaItem{rs_key(s, 0, i), s.first ? s.pv[i] : s.src_v[i], s.first ? s.pw[i] : s.src_w[i]};
}
DEV void rs_store(const CaPoolSort& s, unsigned, unsigned p, const CaItem& e) { s.dst_k[p] = e.key; s.dst_v[p] = e.val; s.dst_w[p] = e.iou; }

// ---- reliability tables ------------------------------------------------------------------------------------------------------------
struct CaTable {
    const u64* keys; const unsigned* flags; const float* iou;            // sorted by (class, score)
    const u64* pool_keys; const unsigned* pool_flags; const float* pool_iou;      // sorted by score
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C, K;
    const int* gt_count; const int* gt_imgs; const int* correct;
    u64* result;
};

// the result block: head, then n, tp (int64), sum_p, sum_iou (float64) [T][C + 1][2][K] each, then brier, nll (float64),
// out_of_range, entries (int64) [T][C + 1] each, then int64 gt_count [C], gt_imgs [C], correct [T][C]
long long ca_result_words(int T, int C, int K) {
    const long long S = (long long)C + 1;
    return CA_RESULT_HEAD + 8ll * T * S * K + 4ll * T * S + 2ll * C + (long long)T * C;
}
bool ca_shape_ok(int T, int C, int K) {
    return T >= 1 && T <= CA_MAX_T && em_classes_ok(C) && K >= 1 && K <= CA_MAX_K && (long long)T * ((long long)C + 1) * K <= CA_MAX_CELLS;
}

// workgroup (s, 3 t + part): scope s at threshold t; part 0 the width bins, 1 the mass bins, 2 the scope's totals and counters
__global__ __launch_bounds__(CA_THREADS) void ca_table_kernel(CaTable a) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ double shd[EV_WAVES];
    __shared__ unsigned blo[CA_MAX_K], bhi[CA_MAX_K];
    const int s = blockIdx.x, t = blockIdx.y / CA_PARTS, part = blockIdx.y % CA_PARTS, tid = threadIdx.x;
    const long long S = (long long)a.C + 1, cells = (long long)a.T * S * 2 * a.K, ts = (long long)t * S + s;
    const unsigned n = ev_live(a.state, a.n_host, a.capacity);
    const bool pooled = s == a.C;
    const u64* keys = pooled ? a.pool_keys : a.keys;
    const unsigned* flags = pooled ? a.pool_flags : a.flags;
    const float* iou = pooled ? a.pool_iou : a.iou;
    const unsigned beg = pooled ? 0u : ev_class_begin(keys, n, s);
    const unsigned end = pooled ? ev_class_begin(keys, n, 1) : ev_class_begin(keys, n, s + 1);
    const unsigned m = end - beg;
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    long long* res_i = reinterpret_cast<long long*>(a.result + CA_RESULT_HEAD);
    double* res_d = reinterpret_cast<double*>(a.result + CA_RESULT_HEAD);
    if (part < 2) {
        const int K = a.K;
        if (tid < K) {
            unsigned lo, hi;
            if (part == 0) {                                              // entries of the bins above k come first
                const u64* seg = keys + beg;
                auto above = [seg, m, K](int q) -> unsigned {
                    if (q < 0) return m;
                    if (q >= K - 1) return 0u;
                    return fo_partition_point(seg, m, [q, K](u64 v) { return ca_bin(ca_score(v), K) > q; });
                };
                lo = above(tid); hi = above(tid - 1);
            } else {
                lo = (unsigned)((u64)tid * m / (u64)K); hi = (unsigned)((u64)(tid + 1) * m / (u64)K);
            }
            blo[tid] = lo; bhi[tid] = hi;
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const unsigned lo = beg + blo[k], hi = beg + bhi[k];          // beg <= lo <= hi <= end <= n
            unsigned cn = 0, ct = 0;
            double sp = 0.0, si = 0.0;
            for (unsigned i = lo + tid; i < hi; i += CA_THREADS) {
                const unsigned f = flags[i];
                if (f & ig_bit) continue;
                ++cn;
                sp = sp + (double)ca_score(keys[i]);
                if (f & tp_bit) { ++ct; si = si + (double)iou[i]; }
            }
            cn = ev_block_sum<unsigned>(cn, shu, tid);
            ct = ev_block_sum<unsigned>(ct, shu, tid);
            sp = ev_block_sum<double>(sp, shd, tid);
            si = ev_block_sum<double>(si, shd, tid);
            if (tid == 0) {
                const long long at = (ts * 2 + part) * K + k;
                res_i[at] = cn; res_i[cells + at] = ct; res_d[2 * cells + at] = sp; res_d[3 * cells + at] = si;
            }
        }
        return;
    }
    unsigned oor = 0;
    double br = 0.0, nl = 0.0;
    for (unsigned i = beg + tid; i < end; i += CA_THREADS) {
        const unsigned f = flags[i];
        if (f & ig_bit) continue;
        const float pf = ca_score(keys[i]);
        const bool tp = f & tp_bit;
        const double p = (double)pf, d = p - (tp ? 1.0 : 0.0), c = ca_clamp(p);
        if (!(pf >= 0.f && pf <= 1.f)) ++oor;
        br = br + d * d;
        nl = nl - log(tp ? c : 1.0 - c);
    }
    oor = ev_block_sum<unsigned>(oor, shu, tid);
    br = ev_block_sum<double>(br, shd, tid);
    nl = ev_block_sum<double>(nl, shd, tid);
    if (tid != 0) return;
    const long long TS = (long long)a.T * S;
    res_d[4 * cells + ts] = br; res_d[4 * cells + TS + ts] = nl; res_i[4 * cells + 2 * TS + ts] = oor; res_i[4 * cells + 3 * TS + ts] = m;
    long long* cnt = res_i + 4 * cells + 4 * TS;
    if (!pooled) {
        cnt[2ll * a.C + (long long)t * a.C + s] = a.correct[(long long)t * a.C + s];
        if (t == 0) { cnt[s] = a.gt_count[s]; cnt[a.C + s] = a.gt_imgs[s]; }
    }
    if (t == 0 && s == 0) {
        u64* res = a.result;
        res[0] = n; res[1] = a.state ? a.state[1] : 0; res[2] = a.state ? a.state[2] : 0; res[3] = (u64)a.T; res[4] = (u64)a.C;
        res[5] = (u64)a.K; res[6] = 0; res[7] = 0;
    }
}

// ---- workspace layout (host): the class sort's buffers, then the pooled sort's, each with the second payload pair -------------------
bool ca_layout(long long capacity, int C, EvLayout* L, EvLayout* P) {
    return ev_layout(capacity, C, 4, 4, L) && ev_layout(capacity, 1, 4, 4, P);
}

// ---- the Platt / temperature fit ---------------------------------------------------------------------------------------------------
struct CaFit {
    const float* scores; const unsigned* flags; const float* iou; const unsigned* cursor; unsigned capacity;
    int t, soft, temperature;
    double* state; double* partials;
};
DEV unsigned ca_fit_groups(unsigned n) { return (n + CA_FIT_CHUNK - 1) / CA_FIT_CHUNK; }

// workgroup g: the sums of the entries [2048 g, 2048 (g + 1)) at the trial point -> partials[g]
__global__ __launch_bounds__(CA_THREADS) void ca_fit_partial_kernel(CaFit a) {
    __shared__ double shd[EV_WAVES];
    const unsigned g = blockIdx.x;
    const int tid = threadIdx.x;
    if (a.state[CA_FROZEN] != 0.0) return;                                // the same for every thread of every workgroup
    const unsigned n = fo_min(a.cursor[0], a.capacity);
    if (g >= ca_fit_groups(n)) return;
    const double ta = a.state[CA_TA], tb = a.state[CA_TB];
    const unsigned skip = CA_INVALID | (1u << (16 + a.t)), tp_bit = 1u << a.t;
    double v[CA_FIT_SUMS];
#pragma unroll
    for (int q = 0; q < CA_FIT_SUMS; ++q) v[q] = 0.0;
    for (int r = 0; r < EV_AP_ITEMS; ++r) {
        const unsigned i = g * CA_FIT_CHUNK + (unsigned)r * CA_THREADS + (unsigned)tid;
        if (i >= n) continue;
        const unsigned f = a.flags[i];
        const float pf = a.scores[i];
        if ((f & skip) || pf != pf) continue;
        const double y = (f & tp_bit) ? (a.soft ? (double)a.iou[i] : 1.0) : 0.0;
        const double x = ca_logit((double)pf);
        const double z = ta * x + tb;
        const double e = exp(-fabs(z));
        const double sg = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        const double d = sg - y, w = sg * (1.0 - sg);
        v[0] = v[0] + ((log1p(e) + fmax(z, 0.0)) - y * z);
        v[1] = v[1] + d * x; v[2] = v[2] + d;
        v[3] = v[3] + (w * x) * x; v[4] = v[4] + w * x; v[5] = v[5] + w;
        v[6] = v[6] + 1.0;
    }
#pragma unroll
    for (int q = 0; q < CA_FIT_SUMS - 1; ++q) v[q] = ev_block_sum<double>(v[q], shd, tid);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < CA_FIT_SUMS; ++q) a.partials[(long long)g * CA_FIT_SUMS + q] = v[q];
    }
}

// one workgroup: the partials in ascending order, then the state machine
__global__ __launch_bounds__(CA_THREADS) void ca_fit_update_kernel(CaFit a) {
    __shared__ double tot[CA_FIT_SUMS];
    const int tid = threadIdx.x;
    double* st = a.state;
    if (st[CA_FROZEN] != 0.0) return;
    const unsigned groups = ca_fit_groups(fo_min(a.cursor[0], a.capacity));
    if (tid < CA_FIT_SUMS) {
        double sum = 0.0;
        for (unsigned g = 0; g < groups; ++g) sum = sum + a.partials[(long long)g * CA_FIT_SUMS + tid];
        tot[tid] = sum;
    }
    __syncthreads();
    if (tid != 0) return;
    const double L = tot[0], ga = tot[1], gb = tot[2], haa = tot[3], hab = tot[4], hbb = tot[5];
    st[CA_ITER] = st[CA_ITER] + 1.0;
    st[CA_COUNT] = tot[6];
    if (st[CA_HAVE] == 0.0) {
        if (!ca_finite(L)) { st[CA_FROZEN] = 1.0; return; }
        st[CA_NLL0] = L;
    } else if (!(ca_finite(L) && L <= st[CA_NLL] * (1.0 + 0x1p-40))) {     // rejected: half the step from the accepted point
        const double lam = st[CA_LAM] * 0.5;
        st[CA_HALV] = st[CA_HALV] + 1.0;
        st[CA_LAM] = lam;
        st[CA_TA] = st[CA_A] + lam * st[CA_DA];
        st[CA_TB] = st[CA_B] + lam * st[CA_DB];
        if (lam < 0x1p-60) st[CA_FROZEN] = 1.0;
        return;
    }
    const double pa = st[CA_TA], pb = st[CA_TB];
    st[CA_A] = pa; st[CA_B] = pb; st[CA_NLL] = L; st[CA_HAVE] = 1.0;
    double da, db;
    bool ok;
    if (a.temperature) {
        ok = haa > 0.0;
        da = -(ga / haa); db = 0.0;
    } else {
        const double det = haa * hbb - hab * hab;
        ok = det > 0.0 && haa > 0.0;
        da = -((hbb * ga - hab * gb) / det); db = -((haa * gb - hab * ga) / det);
    }
    if (!ok || !ca_finite(da) || !ca_finite(db)) { st[CA_FROZEN] = 1.0; return; }
    if (fmax(fabs(da), fabs(db)) <= 0x1p-40 * fmax(1.0, fmax(fabs(pa), fabs(pb)))) { st[CA_CONV] = 1.0; st[CA_FROZEN] = 1.0; return; }
    st[CA_LAM] = 1.0; st[CA_DA] = da; st[CA_DB] = db;
    st[CA_TA] = pa + da; st[CA_TB] = pb + db;
}

struct CaApply { const float* det_in; const int* count; const double* state; int B, max_det; float* det_out; };

// thread (b, j): row j of image b
__global__ __launch_bounds__(CA_THREADS) void ca_apply_kernel(CaApply p) {
    const long long row = (long long)blockIdx.x * CA_THREADS + threadIdx.x;
    if (row >= (long long)p.B * p.max_det) return;
    const int b = (int)(row / p.max_det), j = (int)(row % p.max_det);
    const float* d = p.det_in + row * 6;
    const float v0 = d[0], v1 = d[1], v2 = d[2], v3 = d[3], v5 = d[5];
    float v4 = d[4];
    if (j < p.count[b]) v4 = (float)ca_sigmoid(p.state[CA_A] * ca_logit((double)v4) + p.state[CA_B]);
    float* o = p.det_out + row * 6;
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; o[4] = v4; o[5] = v5;
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int effdet_calibration_match(void* stream, const float* det, const int* det_count, const float* gt_boxes,
                                        const long long* gt_cls, const unsigned char* gt_difficult, int B, int max_det, int M,
                                        int num_classes, const float* thresholds, int num_thresholds, float score_threshold,
                                        unsigned int* flags, float* iou, int* kept, int* gt_count, int* gt_imgs, int* correct_imgs) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !flags || !iou || !kept || !gt_count || !gt_imgs || !correct_imgs)
        return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, CA_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16, ascending, no NaN
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    if (!(score_threshold == score_threshold)) return EFFDET_EINVAL;      // score_threshold is NaN
    const size_t sh = ((size_t)num_classes + 3 * (size_t)M + 8) * sizeof(int);
    if (sh > 64 * 1024) return EFFDET_EINVAL;      // (num_classes + 3 M + 8) ints exceed 64 KiB of LDS
    CaMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_difficult = gt_difficult;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds; a.score_thr = score_threshold;
    for (int t = 0; t < CA_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.flags = flags; a.iou = iou; a.kept = kept; a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    hipLaunchKernelGGL(ca_match_kernel, dim3(B), dim3(CA_THREADS), sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_calibration_append(void* stream, const float* det, const unsigned int* flags, const float* iou, const int* kept,
                                         int B, int max_det, float score_threshold, float* scores, int* classes,
                                         unsigned int* out_flags, float* out_iou, long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !iou || !kept || !scores || !classes || !out_flags || !out_iou || !state)
        return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    if (!(score_threshold == score_threshold)) return EFFDET_EINVAL;      // score_threshold is NaN
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    const CaAppend a{{det, kept, B, max_det, scores, classes, (unsigned)capacity, state}, flags, iou, out_flags, out_iou, score_threshold};
    return ev_append(stream, a);
}

extern "C" long long effdet_calibration_workspace_bytes(long long capacity, int num_classes) {
    EvLayout L, P;
    return ca_layout(capacity, num_classes, &L, &P) ? L.total + P.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_calibration_sorted_offset(long long capacity, int num_classes, int which) {
    EvLayout L, P;
    if (which < 0 || which > 5 || !ca_layout(capacity, num_classes, &L, &P)) return EFFDET_EINVAL;
    const EvLayout& X = which < 3 ? L : P;
    const int last = ev_last(X), w = which % 3;
    return (which < 3 ? 0 : L.total) + (w == 0 ? X.keys[last] : w == 1 ? X.vals[last] : X.extra[last]);
}

extern "C" long long effdet_calibration_result_bytes(int num_thresholds, int num_classes, int bins) {
    if (!ca_shape_ok(num_thresholds, num_classes, bins)) return EFFDET_EINVAL;
    return 8ll * ca_result_words(num_thresholds, num_classes, bins);
}

extern "C" int effdet_calibration_table(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                        const float* iou, long long capacity, long long n, const unsigned int* state,
                                        int num_thresholds, int num_classes, int bins, const int* gt_count, const int* gt_imgs,
                                        const int* correct_imgs, void* workspace, long long workspace_bytes, void* result) {
    EFFDET_ENTER();
    if (!scores || !classes || !flags || !iou || !gt_count || !gt_imgs || !correct_imgs || !workspace || !result)
        return EFFDET_EINVAL;      // null pointer
    if (n < 0 && !state) return EFFDET_EINVAL;      // n < 0 takes the count from `state`, which is null
    if (!ca_shape_ok(num_thresholds, num_classes, bins))
        return EFFDET_EINVAL;      // thresholds in 1..16, classes in 1..65535, bins in 1..64, T (C + 1) K <= 2^20
    EvLayout L, P;
    if (!ca_layout(capacity, num_classes, &L, &P)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    if (n > capacity) return EFFDET_EINVAL;      // n exceeds the capacity
    if (workspace_bytes < L.total + P.total) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(result) % 8)
        return EFFDET_EINVAL;      // workspace and result must be 8-byte aligned
    char* ws = reinterpret_cast<char*>(workspace);
    char* pws = ws + L.total;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long n_host = n < 0 ? -1 : n;
    CaSort s;
    s.flags = flags; s.iou = reinterpret_cast<const unsigned*>(iou); s.src_w = nullptr; s.dst_w = nullptr;
    ev_sort(st, s, scores, classes, state, n_host, capacity, num_classes, ws, L, [ws, &L](CaSort& p, int d) {
        p.src_w = reinterpret_cast<const unsigned*>(ws + L.extra[1 - d]); p.dst_w = reinterpret_cast<unsigned*>(ws + L.extra[d]);
    });
    const int last = ev_last(L), plast = ev_last(P);
    CaTable a;
    a.keys = reinterpret_cast<const u64*>(ws + L.keys[last]); a.flags = reinterpret_cast<const unsigned*>(ws + L.vals[last]);
    a.iou = reinterpret_cast<const float*>(ws + L.extra[last]);
    CaPoolSort q;
    q.pk = a.keys; q.pv = a.flags; q.pw = reinterpret_cast<const unsigned*>(a.iou); q.src_w = nullptr; q.dst_w = nullptr;
    q.num_classes = num_classes;
    ev_sort(st, q, scores, classes, state, n_host, capacity, 1, pws, P, [pws, &P](CaPoolSort& p, int d) {
        p.src_w = reinterpret_cast<const unsigned*>(pws + P.extra[1 - d]); p.dst_w = reinterpret_cast<unsigned*>(pws + P.extra[d]);
    });
    a.pool_keys = reinterpret_cast<const u64*>(pws + P.keys[plast]); a.pool_flags = reinterpret_cast<const unsigned*>(pws + P.vals[plast]);
    a.pool_iou = reinterpret_cast<const float*>(pws + P.extra[plast]);
    a.state = state; a.n_host = n_host; a.capacity = (unsigned)capacity;
    a.T = num_thresholds; a.C = num_classes; a.K = bins;
    a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    a.result = reinterpret_cast<u64*>(result);
    hipLaunchKernelGGL(ca_table_kernel, dim3((unsigned)num_classes + 1, (unsigned)(CA_PARTS * num_thresholds)), dim3(CA_THREADS), 0, st, a);
    return effdet_check_launch();
}

extern "C" long long effdet_calibration_fit_workspace_bytes(long long capacity) {
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;
    return 8ll * CA_FIT_SUMS * ((capacity + CA_FIT_CHUNK - 1) / CA_FIT_CHUNK);
}

extern "C" int effdet_calibration_fit_step(void* stream, const float* scores, const unsigned int* flags, const float* iou,
                                           long long capacity, const unsigned int* state, int threshold_index, int soft_target,
                                           int temperature, double* fit_state, void* workspace, long long workspace_bytes) {
    EFFDET_ENTER();
    if (!scores || !flags || !iou || !state || !fit_state || !workspace) return EFFDET_EINVAL;      // null pointer
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    if (threshold_index < 0 || threshold_index >= CA_MAX_T) return EFFDET_EINVAL;      // 0 <= threshold_index <= 15
    const long long groups = (capacity + CA_FIT_CHUNK - 1) / CA_FIT_CHUNK;
    if (workspace_bytes < 8ll * CA_FIT_SUMS * groups) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(fit_state) % 8)
        return EFFDET_EINVAL;      // workspace and fit_state must be 8-byte aligned
    const CaFit a{scores, flags, iou, state, (unsigned)capacity, threshold_index, soft_target ? 1 : 0, temperature ? 1 : 0, fit_state,
                  reinterpret_cast<double*>(workspace)};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ca_fit_partial_kernel, dim3((unsigned)groups), dim3(CA_THREADS), 0, st, a);
    hipLaunchKernelGGL(ca_fit_update_kernel, dim3(1), dim3(CA_THREADS), 0, st, a);
    return effdet_check_launch();
}

extern "C" int effdet_calibration_apply(void* stream, const float* det_in, const int* count, const double* fit_state, int B,
                                        int max_det, float* det_out) {
    EFFDET_ENTER();
    if (!det_in || !count || !fit_state || !det_out) return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    const CaApply a{det_in, count, fit_state, B, max_det, det_out};
    const unsigned grid = (unsigned)(((long long)B * max_det + CA_THREADS - 1) / CA_THREADS);
    hipLaunchKernelGGL(ca_apply_kernel, dim3(grid), dim3(CA_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}
