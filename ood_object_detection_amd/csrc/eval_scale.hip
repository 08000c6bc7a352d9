// Dataset-scale detection evaluation on the device: the PASCAL-style AP / CorLoc of evaluation.hip for a whole validation set, at
// up to 16 IoU thresholds in one pass.  Compiled with -ffp-contract=off: IoU must round like the reference's separate float32 numpy
// operations (effdet/evaluation/np_box_ops.py), and every float64 term of AP is a division, a subtraction, a product, one rounding each.
//
//   match    one workgroup per image, as eval_match_kernel: detections in descending score order, each takes the ground-truth box of
//            its class with the largest IoU (first on ties; `difficult` boxes take part).  That candidate does not depend on the
//            threshold, so one serial walk serves all T thresholds: a T-bit `taken` mask per box; a detection whose candidate is
//            difficult is IGNORED at the thresholds its IoU reaches (per_image_evaluation.py:391-407, :471).  One flag word per slot.
//   append   (score, class, flag word) of the valid slots -> capacity-sized buffers at a cursor that lives on the device, in (image,
//            slot) order: the images' kept counts come from the match launch, a workgroup adds up the counts of the images before
//            its own, a one-workgroup launch moves the cursor.  No atomic decides a position.  (ev_append of eval_sorted.h, which
//            states the accumulate stage once for this unit and coco_eval.hip: reductions, append, key, layout, passes.)
//   sort     the stable LSD radix sort of radix_sort.h over 48-bit keys (class, then score descending) with the flag word as payload,
//            five passes, six beyond 255 classes.  Equal scores keep their arrival order; every class is one contiguous segment;
//            invalid entries sort behind the last class.
//   AP       one workgroup per (class, threshold) over its segment: the totals first, then the 2048-entry chunks from the last to the
//            first: rank and cumulative TP by an integer scan, precision = ctp / rank in float64, the VOC envelope by a reverse
//            max-scan carried from chunk to chunk (a maximum: exact), AP = sum over the true positives of (recall step) * envelope
//            in a fixed order.  No floating-point atomics; the same sorted input gives the same bits.
//   open     the open-set protocol on the same pipeline, the last class being "unknown": an open word per kept known-class
//            detection (bit t: its largest IoU with the image's unknown boxes reaches threshold t) travels through the append and the
//            sort as a second payload word; after the same AP launch one workgroup per (class, threshold) counts detections, true
//            positives and open detections, in total and up to the position at which recall is nearest a level (integers only).
//            A one-launch kernel relabels detections below a score threshold as unknown.
//
// Launch boundaries are the only synchronisation between workgroups.  Every loop has a trip count known at its entry, every scatter
// index is compared with the live count before the store; the live count is read from the device cursor (grids are sized by the
// capacity; workgroups beyond the live count exit), so the host never reads anything back.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"
#include "eval_match.h"
#include "eval_sorted.h"

namespace {

constexpr int ES_THREADS = EV_THREADS;
constexpr int ES_MAX_T = 16;
constexpr unsigned ES_INVALID = 0x80000000u;
constexpr int ES_RESULT_HEAD = 8;                                 // 8-byte words before the AP matrix

// ---- matching --------------------------------------------------------------------------------------------------------------------
struct EsMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls; const unsigned char* gt_difficult;
    int B, max_det, M, C, T; float thr[ES_MAX_T];
    unsigned* flags; int* kept; int* gt_count; int* gt_imgs; int* correct;
};

__global__ __launch_bounds__(ES_THREADS) void es_match_kernel(EsMatch p) {
    extern __shared__ int sh[];
    int* seen = sh;                                  // [C] class already had its top-scoring detection
    int* taken = sh + p.C;                           // [M] bit t: taken at threshold t
    int* gcls = taken + p.M;                         // [M] 0-based class or -1
    int* gdif = gcls + p.M;                          // [M]
    float* red_v = reinterpret_cast<float*>(gdif + p.M);    // [4]
    int* red_i = reinterpret_cast<int*>(red_v + 4);          // [4]
    const int b = blockIdx.x, tid = threadIdx.x;
    em_stage_gt(p.gt_cls, p.gt_difficult, b, p.M, p.C, seen, taken, gcls, gdif, p.gt_count, p.gt_imgs);      // difficult boxes: not in gt_count
    const int n = min(p.det_count[b], p.max_det);
    int kept = 0, nans = 0;                          // thread 0's
    for (int i = 0; i < p.max_det; ++i) {
        unsigned* out = p.flags + (long long)b * p.max_det + i;
        if (i >= n) { if (tid == 0) *out = ES_INVALID; continue; }
        const float* d = p.det + ((long long)b * p.max_det + i) * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4];
        const int c = (int)d[5] - 1;
        if (score != score) ++nans;
        if (!(y1 < y2 && x1 < x2) || c < 0 || c >= p.C || score != score) { if (tid == 0) *out = ES_INVALID; continue; }     // uniform
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
            *out = word;
            if (!(word & ES_INVALID)) ++kept;             // T = 16: ignored at all 16 thresholds = bit 31 = dropped, the same thing
            if (!seen[c]) {                                                          // top-scoring detection of class c
                seen[c] = 1;
                for (int t = 0; t < p.T; ++t)
                    if ((reach >> t) & 1u) atomicAdd(p.correct + (long long)t * p.C + c, 1);
            }
        }
        __syncthreads();
    }
    if (tid == 0 && p.kept) { p.kept[b] = kept; p.kept[p.B + b] = nans; }
}

// ---- append: the flag word travels with (score, class), and the open word (null: none) at the same position ---------------------
struct EsAppend : EvAppend { const unsigned* flags; unsigned* out_flags; const unsigned* open; unsigned* out_open; };
DEV bool ev_keep(const EsAppend& a, long long slot, unsigned* word) { *word = a.flags[slot]; return !(*word & ES_INVALID); }
DEV void ev_store(const EsAppend& a, long long slot, unsigned p, unsigned word) {
    a.out_flags[p] = word;
    if (a.out_open) a.out_open[p] = a.open[slot];
}

// ---- sort: the pass descriptor of radix_sort.h (W2: a second payload word, the open word) ------------------------------------------
template <bool W2> struct EsItem { u64 key; unsigned val; };
template <> struct EsItem<true> { u64 key; unsigned val, open; };
template <bool W2> struct EsSort : EvSort {
    typedef EsItem<W2> Item;
    const unsigned* flags;                                                // the first pass reads these
    const unsigned* open; const unsigned* src_w; unsigned* dst_w;         // W2 only
};
// an entry whose flag word has bit 31 is not valid
template <bool W2> DEV u64 rs_key(const EsSort<W2>& s, unsigned, unsigned i) {
    return ev_key(s, i, [&s](unsigned k) { return !(s.flags[k] & ES_INVALID); });
}
template <bool W2> DEV EsItem<W2> rs_load(const EsSort<W2>& s, unsigned, unsigned i) {
    EsItem<W2> e;
    e.key = rs_key(s, 0, i);
    e.val = s.first ? s.flags[i] : s.src_v[i];
    if constexpr (W2) e.open = s.first ? s.open[i] : s.src_w[i];
    return e;
}
template <bool W2> DEV void rs_store(const EsSort<W2>& s, unsigned, unsigned p, const EsItem<W2>& e) {
    s.dst_k[p] = e.key; s.dst_v[p] = e.val;
    if constexpr (W2) s.dst_w[p] = e.open;
}

// ---- average precision -----------------------------------------------------------------------------------------------------------
struct EsAp {
    const u64* keys; const unsigned* flags;                               // sorted
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C;
    const int* gt_count; const int* gt_imgs; const int* correct;
    u64* result;
};

// workgroup (c, t): AP of class c at threshold t, and the (c, t) entries of the result block
__global__ __launch_bounds__(ES_THREADS) void es_ap_kernel(EsAp a) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ double shd[EV_WAVES];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const unsigned n = ev_live(a.state, a.n_host, a.capacity);
    const unsigned s = ev_class_begin(a.keys, n, c), e = ev_class_begin(a.keys, n, c + 1);
    const int ng = a.gt_count[c];
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    double acc = 0.0;
    if (ng > 0 && e > s) {                                                // the same for the whole workgroup
        unsigned tot = 0;                                                 // not ignored | true positives << 16 per thread: < 2^16 each
        unsigned rem_ni = 0, rem_tp = 0;
        for (unsigned i0 = s; i0 < e; i0 += ES_THREADS * 256) {           // a thread adds up to 256 entries before the sums are unpacked
            tot = 0;
            unsigned i = i0 + tid;
            for (unsigned r = 0; r < 256 && i < e; ++r, i += ES_THREADS) {
                const unsigned f = a.flags[i];
                tot += ((f & ig_bit) ? 0u : 1u) + ((f & tp_bit) ? 0x10000u : 0u);
            }
            rem_ni += ev_block_sum<unsigned>(tot & 0xFFFFu, shu, tid);
            rem_tp += ev_block_sum<unsigned>(tot >> 16, shu, tid);
        }
        const double dng = (double)ng;
        double carry = 0.0;                                               // largest precision of the chunks behind this one
        const unsigned nchunks = (e - s + EV_AP_CHUNK - 1) / EV_AP_CHUNK;
        for (unsigned q = nchunks; q-- > 0;) {
            const unsigned i0 = s + q * EV_AP_CHUNK + (unsigned)tid * EV_AP_ITEMS;
            unsigned f[EV_AP_ITEMS], cnt = 0;
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r) {
                f[r] = i0 + r < e ? a.flags[i0 + r] : ig_bit;              // beyond the segment: ignored
                cnt += ((f[r] & ig_bit) ? 0u : 1u) + ((f[r] & tp_bit) ? 0x10000u : 0u);
            }
            unsigned total;
            const unsigned ex = fo_block_excl_scan(cnt, shu, tid, &total);
            rem_ni -= total & 0xFFFFu; rem_tp -= total >> 16;             // now: the counts in front of this chunk
            unsigned rank = rem_ni + (ex & 0xFFFFu), ctp = rem_tp + (ex >> 16);
            double prec[EV_AP_ITEMS], step[EV_AP_ITEMS];
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r) {
                const bool ni = !(f[r] & ig_bit), tp = f[r] & tp_bit;
                rank += ni ? 1u : 0u; ctp += tp ? 1u : 0u;
                prec[r] = ni ? (double)ctp / (double)rank : 0.0;
                step[r] = tp ? (double)ctp / dng - (double)(ctp - 1u) / dng : 0.0;
            }
#pragma unroll
            for (int r = EV_AP_ITEMS - 2; r >= 0; --r) prec[r] = fmax(prec[r], prec[r + 1]);      // envelope inside the thread
            double chunk_max;
            const double later = fmax(ev_block_excl_rmax(prec[0], shd, tid, &chunk_max), carry);
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r)
                if (f[r] & tp_bit) sum += step[r] * fmax(prec[r], later);
            acc += ev_block_sum<double>(sum, shd, tid);
            carry = fmax(carry, chunk_max);
        }
    }
    if (tid != 0) return;
    u64* res = a.result;
    double* ap = reinterpret_cast<double*>(res + ES_RESULT_HEAD);
    long long* cnt = reinterpret_cast<long long*>(res + ES_RESULT_HEAD + (long long)a.T * a.C);
    ap[(long long)t * a.C + c] = ng > 0 ? acc : __builtin_nan("");
    cnt[2ll * a.C + (long long)t * a.C + c] = a.correct[(long long)t * a.C + c];
    if (t == 0) { cnt[c] = ng; cnt[a.C + c] = a.gt_imgs[c]; }
    if (t == 0 && c == 0) {
        res[0] = n; res[1] = a.state ? a.state[1] : 0; res[2] = a.state ? a.state[2] : 0; res[3] = (u64)a.T; res[4] = (u64)a.C;
        res[5] = 0; res[6] = 0; res[7] = 0;
    }
}

// ---- open-set protocol: known classes 0 .. C-2, the unknown class U = C-1 (0-based) -------------------------------------------------
constexpr int ES_OPEN_CHUNK = ES_THREADS;                             // unknown boxes staged in LDS at a time
constexpr int ES_OPEN_MATS = 7;                                       // n_det, tp, open_total, k_star, pos, rank_at, open_at

struct EsOpenWords {
    const float* det; const unsigned* flags; const float* gt_boxes; const long long* gt_cls;
    int B, max_det, M, U, T; float thr[ES_MAX_T];                     // U: the 1-based unknown class
    unsigned* open;
};

// workgroup b: bit t of a kept known-class detection = its largest IoU with the image's boxes of class U reaches thr[t].  No greedy
// state: a detection per thread; the unknown boxes pass through LDS ES_OPEN_CHUNK ground-truth rows at a time, compacted, so every
// thread reads the same LDS word (a broadcast).  A maximum over `>` does not depend on the order of the boxes.
__global__ __launch_bounds__(ES_THREADS) void es_open_words_kernel(EsOpenWords p) {
    __shared__ float box[ES_OPEN_CHUNK][4];
    __shared__ unsigned shu[EV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i0 = 0; i0 < p.max_det; i0 += ES_THREADS) {
        const int i = i0 + tid;
        const long long slot = (long long)b * p.max_det + i;
        bool live = false;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
        if (i < p.max_det) {
            const float* d = p.det + slot * 6;
            const int c1 = (int)d[5];
            live = !(p.flags[slot] & ES_INVALID) && c1 >= 1 && c1 < p.U;
            x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
        }
        const EmDet d = em_det(x1, y1, x2, y2);
        float best = -__builtin_inff();
        for (int j0 = 0; j0 < p.M; j0 += ES_OPEN_CHUNK) {             // uniform trip count
            const int j = j0 + tid;
            const bool unk = j < p.M && p.gt_cls[(long long)b * p.M + j] == (long long)p.U;
            unsigned cnt;
            const unsigned at = fo_block_excl_scan(unk ? 1u : 0u, shu, tid, &cnt);      // at < ES_OPEN_CHUNK
            if (unk) {
                const float* g = p.gt_boxes + ((long long)b * p.M + j) * 4;
                box[at][0] = g[0]; box[at][1] = g[1]; box[at][2] = g[2]; box[at][3] = g[3];
            }
            __syncthreads();
            if (live)
                for (unsigned k = 0; k < cnt; ++k) {
                    const float iou = em_iou(d, box[k][0], box[k][1], box[k][2], box[k][3]);      // yxyx
                    if (iou > best) best = iou;
                }
            __syncthreads();                                          // the chunk is free again
        }
        if (i < p.max_det) {
            unsigned word = 0;
            if (live)
                for (int t = 0; t < p.T; ++t) word |= (best >= p.thr[t] ? 1u : 0u) << t;
            p.open[slot] = word;
        }
    }
}

struct EsOpenCounts {
    const u64* keys; const unsigned* flags; const unsigned* open;        // sorted
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C; double level;
    const int* gt_count;
    long long* mats;                                                      // [ES_OPEN_MATS][T][C]
};

// entries [s, e) of one segment: not ignored at t, true positives at t, open bit t (three sums in a fixed order)
DEV void es_open_totals(const EsOpenCounts& a, unsigned s, unsigned e, unsigned tp_bit, unsigned ig_bit, unsigned* shu, int tid,
                        unsigned* ni, unsigned* tp, unsigned* op) {
    unsigned c_ni = 0, c_tp = 0, c_op = 0;                                // a thread sees at most 2^24 / 256 entries
    for (unsigned i = s + tid; i < e; i += ES_THREADS) {
        const unsigned f = a.flags[i];
        c_ni += (f & ig_bit) ? 0u : 1u; c_tp += (f & tp_bit) ? 1u : 0u; c_op += (a.open[i] & tp_bit) ? 1u : 0u;
    }
    *ni = ev_block_sum<unsigned>(c_ni, shu, tid);
    *tp = ev_block_sum<unsigned>(c_tp, shu, tid);
    *op = ev_block_sum<unsigned>(c_op, shu, tid);
}

// workgroup (c, t): the counts of class c at threshold t.  Pass 1: the totals, then k_star = the reachable cumulative-TP count
// whose recall is nearest the level (float64, ties to the smaller count; the candidates floor(level n_gt) - 1 .. + 2 suffice).
// Pass 2: the first position with that count (the chunks from the front, an integer scan each), and the counts up to it.
__global__ __launch_bounds__(ES_THREADS) void es_open_counts_kernel(EsOpenCounts a) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ unsigned sh_pos;
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const unsigned n = ev_live(a.state, a.n_host, a.capacity);
    const unsigned s = ev_class_begin(a.keys, n, c), e = ev_class_begin(a.keys, n, c + 1);
    const int ng = a.gt_count[c];
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    unsigned n_det, tp, open_total;
    es_open_totals(a, s, e, tp_bit, ig_bit, shu, tid, &n_det, &tp, &open_total);
    long long k_star = 0, pos = -1, rank_at = 0, open_at = 0;
    if (ng > 0 && e > s) {                                                // the same for the whole workgroup
        const long long k_min = (a.flags[s] & tp_bit) ? 1 : 0, k_max = (long long)tp;
        const double dng = (double)ng;
        const long long base = (long long)floor(a.level * dng);
        double best = 0.0;
        bool have = false;
        for (long long d = -1; d <= 2; ++d) {
            long long k = base + d;
            k = k < k_min ? k_min : (k > k_max ? k_max : k);              // ascending in d: the first minimum is the smaller count
            const double dist = fabs((double)k / dng - a.level);
            if (!have || dist < best) { best = dist; k_star = k; have = true; }
        }
        unsigned first = s;                                               // k_star = 0: position 0 (k_min is 0 then)
        if (k_star > 0) {
            const unsigned want = (unsigned)k_star;
            unsigned seen = 0;
            bool found = false;
            const unsigned nchunks = (e - s + EV_AP_CHUNK - 1) / EV_AP_CHUNK;
            for (unsigned q = 0; q < nchunks && !found; ++q) {            // `found` is the same for the whole workgroup
                const unsigned i0 = s + q * EV_AP_CHUNK + (unsigned)tid * EV_AP_ITEMS;
                unsigned f[EV_AP_ITEMS], cnt = 0;
#pragma unroll
                for (int r = 0; r < EV_AP_ITEMS; ++r) {
                    f[r] = i0 + r < e ? a.flags[i0 + r] : 0u;
                    cnt += (f[r] & tp_bit) ? 1u : 0u;
                }
                unsigned total;
                unsigned run = seen + fo_block_excl_scan(cnt, shu, tid, &total);
                if (run < want && want <= run + cnt) {                    // one thread of one chunk
#pragma unroll
                    for (int r = 0; r < EV_AP_ITEMS; ++r) {
                        if (f[r] & tp_bit) { ++run; if (run == want) sh_pos = i0 + r; }
                    }
                }
                __syncthreads();
                found = seen + total >= want;
                if (found) first = sh_pos;
                seen += total;
            }
        }
        pos = (long long)(first - s);
        unsigned ni_at, tp_at, op_at;
        es_open_totals(a, s, first + 1, tp_bit, ig_bit, shu, tid, &ni_at, &tp_at, &op_at);
        rank_at = ni_at; open_at = op_at;
    }
    if (tid != 0) return;
    const long long TC = (long long)a.T * a.C, at = (long long)t * a.C + c;
    a.mats[0 * TC + at] = n_det; a.mats[1 * TC + at] = tp; a.mats[2 * TC + at] = open_total;
    a.mats[3 * TC + at] = k_star; a.mats[4 * TC + at] = pos; a.mats[5 * TC + at] = rank_at; a.mats[6 * TC + at] = open_at;
}

// ---- relabelling below a score threshold --------------------------------------------------------------------------------------------
struct EsRelabel {
    const float* det_in; const int* count; const float* score; long long pitch, stride;
    int B, max_det, C; float tau; const float* tau_dev; float* det_out;
};

// thread (b, j): row j of image b, its class set to C + 1 where j < count[b], the class is in 1..C and !(score >= tau)
__global__ __launch_bounds__(ES_THREADS) void es_relabel_unknown_kernel(EsRelabel p) {
    const long long row = (long long)blockIdx.x * ES_THREADS + threadIdx.x;
    if (row >= (long long)p.B * p.max_det) return;
    const int b = (int)(row / p.max_det), j = (int)(row % p.max_det);
    const float tau = p.tau_dev ? p.tau_dev[0] : p.tau;
    const float* d = p.det_in + row * 6;
    const float v0 = d[0], v1 = d[1], v2 = d[2], v3 = d[3], v4 = d[4];
    float cls = d[5];
    const int c1 = (int)cls;
    if (j < p.count[b] && c1 >= 1 && c1 <= p.C && !(p.score[(long long)b * p.pitch + (long long)j * p.stride] >= tau))
        cls = (float)(p.C + 1);
    float* o = p.det_out + row * 6;
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; o[4] = v4; o[5] = cls;
}

// ---- workspace layout (host): the sort's buffers, then the second payload pair when there are open words ---------------------------
bool es_layout(long long capacity, int C, EvLayout* L, bool open = false) { return ev_layout(capacity, C, open ? 4 : 0, open ? 4 : 0, L); }

template <bool W2> void es_sort(hipStream_t st, const float* scores, const int* classes, const unsigned* flags, const unsigned* open,
                                const unsigned* state, long long n_host, long long capacity, int C, char* ws, const EvLayout& L) {
    EsSort<W2> s;
    s.flags = flags; s.open = open; s.src_w = nullptr; s.dst_w = nullptr;
    ev_sort(st, s, scores, classes, state, n_host, capacity, C, ws, L, [ws, &L](EsSort<W2>& p, int d) {
        if (!W2) return;
        p.src_w = reinterpret_cast<const unsigned*>(ws + L.extra[1 - d]); p.dst_w = reinterpret_cast<unsigned*>(ws + L.extra[d]);
    });
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int effdet_eval_scale_sort_tile(void) { return RS_TILE; }

extern "C" int effdet_eval_match_multi(void* stream, const float* det, const int* det_count, const float* gt_boxes,
                                       const long long* gt_cls, const unsigned char* gt_difficult, int B, int max_det, int M,
                                       int num_classes, const float* thresholds, int num_thresholds, unsigned int* flags, int* kept,
                                       int* gt_count, int* gt_imgs, int* correct_imgs) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !flags || !gt_count || !gt_imgs || !correct_imgs)
        return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, ES_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16, ascending, no NaN
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    const size_t sh = ((size_t)num_classes + 3 * (size_t)M + 8) * sizeof(int);
    if (sh > 64 * 1024) return EFFDET_EINVAL;      // (num_classes + 3 M + 8) ints exceed 64 KiB of LDS
    EsMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_difficult = gt_difficult;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds;
    for (int t = 0; t < ES_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.flags = flags; a.kept = kept; a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    hipLaunchKernelGGL(es_match_kernel, dim3(B), dim3(ES_THREADS), sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_eval_append(void* stream, const float* det, const unsigned int* flags, const int* kept, int B, int max_det,
                                  float* scores, int* classes, unsigned int* out_flags, long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !kept || !scores || !classes || !out_flags || !state) return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    const EsAppend a{{det, kept, B, max_det, scores, classes, (unsigned)capacity, state}, flags, out_flags, nullptr, nullptr};
    return ev_append(stream, a);
}

extern "C" int effdet_eval_append_open(void* stream, const float* det, const unsigned int* flags, const unsigned int* open,
                                       const int* kept, int B, int max_det, float* scores, int* classes, unsigned int* out_flags,
                                       unsigned int* out_open, long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !open || !kept || !scores || !classes || !out_flags || !out_open || !state)
        return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    const EsAppend a{{det, kept, B, max_det, scores, classes, (unsigned)capacity, state}, flags, out_flags, open, out_open};
    return ev_append(stream, a);
}

extern "C" long long effdet_eval_ap_sorted_workspace_bytes(long long capacity, int num_classes) {
    EvLayout L;
    return es_layout(capacity, num_classes, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_eval_ap_sorted_offset(long long capacity, int num_classes, int which) {
    EvLayout L;
    if ((which != 0 && which != 1) || !es_layout(capacity, num_classes, &L)) return EFFDET_EINVAL;
    return which == 0 ? L.keys[ev_last(L)] : L.vals[ev_last(L)];
}

extern "C" long long effdet_eval_ap_sorted_result_bytes(int num_thresholds, int num_classes) {
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T || !em_classes_ok(num_classes)) return EFFDET_EINVAL;
    return 8ll * (ES_RESULT_HEAD + 2ll * num_thresholds * num_classes + 2ll * num_classes);
}

// sort + AP (+ the open-set counts when `open` is given): the body of effdet_eval_ap_sorted and effdet_eval_open_sorted
static int es_sorted_run(void* stream, const float* scores, const int* classes, const unsigned int* flags, const unsigned int* open,
                         long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes,
                         const int* gt_count, const int* gt_imgs, const int* correct_imgs, double level, void* workspace,
                         long long workspace_bytes, void* result) {
    if (!scores || !classes || !flags || !gt_count || !gt_imgs || !correct_imgs || !workspace || !result)
        return EFFDET_EINVAL;      // null pointer
    if (n < 0 && !state) return EFFDET_EINVAL;      // n < 0 takes the count from `state`, which is null
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    EvLayout L;
    if (!es_layout(capacity, num_classes, &L, open != nullptr)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    if (n > capacity) return EFFDET_EINVAL;      // n exceeds the capacity
    if (workspace_bytes < L.total) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(result) % 8)
        return EFFDET_EINVAL;      // workspace and result must be 8-byte aligned
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long n_host = n < 0 ? -1 : n;
    if (open) es_sort<true>(st, scores, classes, flags, open, state, n_host, capacity, num_classes, ws, L);
    else es_sort<false>(st, scores, classes, flags, nullptr, state, n_host, capacity, num_classes, ws, L);
    const int last = ev_last(L);
    EsAp a;
    a.keys = reinterpret_cast<const u64*>(ws + L.keys[last]); a.flags = reinterpret_cast<const unsigned*>(ws + L.vals[last]);
    a.state = state; a.n_host = n_host; a.capacity = (unsigned)capacity;
    a.T = num_thresholds; a.C = num_classes;
    a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    a.result = reinterpret_cast<u64*>(result);
    hipLaunchKernelGGL(es_ap_kernel, dim3((unsigned)num_classes, (unsigned)num_thresholds), dim3(ES_THREADS), 0, st, a);
    if (open) {
        EsOpenCounts o;
        o.keys = a.keys; o.flags = a.flags; o.open = reinterpret_cast<const unsigned*>(ws + L.extra[last]);
        o.state = state; o.n_host = n_host; o.capacity = (unsigned)capacity;
        o.T = num_thresholds; o.C = num_classes; o.level = level;
        o.gt_count = gt_count;
        o.mats = reinterpret_cast<long long*>(result) + ES_RESULT_HEAD + 2ll * num_thresholds * num_classes + 2ll * num_classes;
        hipLaunchKernelGGL(es_open_counts_kernel, dim3((unsigned)num_classes, (unsigned)num_thresholds), dim3(ES_THREADS), 0, st, o);
    }
    return effdet_check_launch();
}

extern "C" int effdet_eval_ap_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                     long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes,
                                     const int* gt_count, const int* gt_imgs, const int* correct_imgs, void* workspace,
                                     long long workspace_bytes, void* result) {
    EFFDET_ENTER();
    return es_sorted_run(stream, scores, classes, flags, nullptr, capacity, n, state, num_thresholds, num_classes, gt_count, gt_imgs,
                         correct_imgs, 0.0, workspace, workspace_bytes, result);
}

// ---- open-set protocol: C ABI (num_classes counts the unknown class: known classes 1 .. num_classes - 1) -----------------------------
extern "C" int effdet_eval_open_words(void* stream, const float* det, const unsigned int* flags, const float* gt_boxes,
                                      const long long* gt_cls, int B, int max_det, int M, int num_classes, const float* thresholds,
                                      int num_thresholds, unsigned int* open) {
    EFFDET_ENTER();
    if (!det || !flags || !gt_boxes || !gt_cls || !thresholds || !open) return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, ES_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16, ascending, no NaN
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (!em_classes_ok(num_classes, 2)) return EFFDET_EINVAL;      // 2 <= num_classes <= 65535
    EsOpenWords a;
    a.det = det; a.flags = flags; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls;
    a.B = B; a.max_det = max_det; a.M = M; a.U = num_classes; a.T = num_thresholds;
    for (int t = 0; t < ES_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.open = open;
    hipLaunchKernelGGL(es_open_words_kernel, dim3(B), dim3(ES_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" long long effdet_eval_open_sorted_workspace_bytes(long long capacity, int num_classes) {
    EvLayout L;
    return es_layout(capacity, num_classes, &L, true) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_eval_open_sorted_offset(long long capacity, int num_classes, int which) {
    EvLayout L;
    if (which < 0 || which > 2 || !es_layout(capacity, num_classes, &L, true)) return EFFDET_EINVAL;
    return which == 0 ? L.keys[ev_last(L)] : which == 1 ? L.vals[ev_last(L)] : L.extra[ev_last(L)];
}

extern "C" long long effdet_eval_open_sorted_result_bytes(int num_thresholds, int num_classes) {
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T || !em_classes_ok(num_classes, 2)) return EFFDET_EINVAL;
    return 8ll * (ES_RESULT_HEAD + (2ll + ES_OPEN_MATS) * num_thresholds * num_classes + 2ll * num_classes);
}

extern "C" int effdet_eval_open_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                       const unsigned int* open, long long capacity, long long n, const unsigned int* state,
                                       int num_thresholds, int num_classes, const int* gt_count, const int* gt_imgs,
                                       const int* correct_imgs, double recall_level, void* workspace, long long workspace_bytes,
                                       void* result) {
    EFFDET_ENTER();
    if (!open) return EFFDET_EINVAL;      // null pointer
    if (num_classes < 2) return EFFDET_EINVAL;      // 2 <= num_classes <= 65535
    if (!(recall_level > 0.0 && recall_level <= 1.0)) return EFFDET_EINVAL;      // recall_level must lie in (0, 1]
    return es_sorted_run(stream, scores, classes, flags, open, capacity, n, state, num_thresholds, num_classes, gt_count, gt_imgs,
                         correct_imgs, recall_level, workspace, workspace_bytes, result);
}

extern "C" int effdet_relabel_unknown(void* stream, const float* det_in, const int* count, const float* score, long long pitch,
                                      long long stride, int B, int max_det, int num_known, float tau, const float* tau_device,
                                      float* det_out) {
    EFFDET_ENTER();
    if (!det_in || !count || !score || !det_out) return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    if (num_known < 1 || num_known >= EM_MAX_C) return EFFDET_EINVAL;      // 1 <= num_known <= 65534
    if (pitch < 0 || stride < 0) return EFFDET_EINVAL;      // negative pitch or stride
    EsRelabel a{det_in, count, score, pitch, stride, B, max_det, num_known, tau, tau_device, det_out};
    const unsigned grid = (unsigned)(((long long)B * max_det + ES_THREADS - 1) / ES_THREADS);
    hipLaunchKernelGGL(es_relabel_unknown_kernel, dim3(grid), dim3(ES_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}
