// OpenImages detection evaluation on the device: the PASCAL protocol of eval_scale.hip with group-of boxes, a
// weight for them, the Challenge's verified image-level labels and the weighted (pooled) mean AP, at up to 15 IoU thresholds from
// one matching pass.  Compiled with -ffp-contract=off: IoU and IoA round like the reference's separate float32 numpy operations
// (effdet/evaluation/np_box_ops.py), every float64 term of AP is one product, one sum or one division, one rounding each.
//
// Definitions (restated in tests/_eval_openimages_ref.py).  Per image: det [max_det][6] rows x1, y1, x2, y2, score, 1-based class in
// descending score order, count valid rows; ground-truth boxes yxyx with a 1-based class (<= 0: padding), a `difficult` flag and a
// `group-of` flag (either table may be null: no box is); labeled_cls [K] int64 1-based verified image-level labels (<= 0:
// padding; a null list: every class is evaluatable in every image).
//   valid     slot i is valid iff i < count, the box is not degenerate, the class lies in 1..C and the score is not NaN.
//   labels    with a list, a valid slot whose class is neither the class of a box of the image nor in the list is dropped: it is
//             no false positive and not the class's top-scoring detection (detection_evaluator.py:568-572).
//   stage 1   the candidate is the box of the class that is not group-of with the largest IoU, the first on ties; `difficult`
//             boxes take part.  IoU >= thr and the candidate difficult: ignored; IoU >= thr and the candidate not taken at thr:
//             true positive, the candidate is taken; otherwise so far a false positive (per_image_evaluation.py:391-407).
//   stage 2   a slot that is neither a true positive nor ignored at thr looks at the class's group-of boxes: the candidate is the
//             one with the largest IoA (intersection over the detection's area), the first on ties; IoA >= thr: the slot is
//             absorbed (its ignore bit is set) and the box remembers the largest absorbed score (:423-434).
//   virtual   a group-of box whose remembered score at thr is > 0 gives, when the weight is > 0, one entry (that score, the box's
//             class, flag word = true positive at thr | ignored at every other threshold | OI_GROUP) per threshold (:435-437).
//   counters  n_plain[c]: boxes neither difficult nor group-of; n_group[c]: group-of boxes that are not difficult; gt_imgs[c]:
//             images with a box of class c; correct[t][c]: images whose top-scoring detection of class c reaches thr[t] by IoU
//             with any box of the class, group-of boxes included (object_detection_evaluation.py:132-139).
//   A box that is both difficult and group-of absorbs detections like any group-of box and is counted nowhere.
//   AP        num_gt = n_plain + w n_group.  Over a class's entries not ignored at thr, by descending score (equal scores in
//             arrival order): rank, a = the plain true positives and g = the group true positives at or before the entry,
//             ctp = a + w g, precision = ctp / (ctp + (rank - a - g)), the VOC envelope, AP = the sum over the true positives of
//             (ctp / num_gt - ctp_before / num_gt) * envelope (metrics.py:4-89).  NaN where num_gt = 0.
//   pooled    the same over the entries of all classes with num_gt > 0, equal scores by (class, arrival), num_gt = the sum.
//
// Launches: match (a workgroup per image: flag word per slot, M T virtual slots, kept and NaN counts, integer counters), append
// (the image's kept slots, then its virtual entries in (box, threshold) order, at the device cursor: ev_append's positions), the
// sort of eval_sorted.h, AP (a workgroup per (class, threshold)); for the pooled AP the same sort again over the class-sorted
// entries with the class replaced by "its class has no instances", and one workgroup per threshold over the one segment.
// Every loop has a trip count known at its entry, every scatter index is compared with the live count, no floating-point atomics,
// nothing is read back: the unit is capturable and gives the same bits for every split into batches.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"
#include "eval_match.h"
#include "eval_sorted.h"

namespace {

constexpr int OI_THREADS = EV_THREADS;
constexpr int OI_MAX_T = 15;                                      // bit 15 of a flag word is the group marker
constexpr unsigned OI_INVALID = 0x80000000u;
constexpr unsigned OI_GROUP = 1u << 15;                           // a virtual entry: a group-of box that absorbed a detection
constexpr int OI_DIFFICULT = 1, OI_GROUP_OF = 2;                  // box bits
constexpr int OI_RESULT_HEAD = 8;                                 // 8-byte words before the AP matrix

// ---- matching --------------------------------------------------------------------------------------------------------------------
struct OiMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls;
    const unsigned char* gt_difficult; const unsigned char* gt_group_of; const long long* labeled_cls;
    int B, max_det, M, C, T, K, emit; float thr[OI_MAX_T];
    unsigned* flags; float* vscore; unsigned* vflags; int* kept; int* n_plain; int* n_group; int* gt_imgs; int* correct;
};

long long oi_match_lds(int M, int C, int T) {
    if (M < 1 || !em_classes_ok(C) || T < 1 || T > OI_MAX_T) return EFFDET_EINVAL;
    return 4ll * ((long long)C + (C + 31) / 32 + 3ll * M + (long long)M * T + 24);
}

__global__ __launch_bounds__(OI_THREADS) void oi_match_kernel(OiMatch p) {
    extern __shared__ int oi_lds[];
    const int W = (p.C + 31) >> 5;
    int* seen = oi_lds;                                           // [C] class already had its top-scoring detection
    unsigned* labset = reinterpret_cast<unsigned*>(seen + p.C);   // [W] evaluatable classes: the boxes' classes and the list
    int* taken = reinterpret_cast<int*>(labset + W);              // [M] bit t: taken at threshold t
    int* gcls = taken + p.M;                                      // [M] 0-based class or -1
    int* gflag = gcls + p.M;                                      // [M] OI_DIFFICULT | OI_GROUP_OF
    float* gscore = reinterpret_cast<float*>(gflag + p.M);        // [M][T] the largest score absorbed at threshold t
    float* red_v = gscore + (long long)p.M * p.T;                 // [4][3]
    int* red_i = reinterpret_cast<int*>(red_v + 12);              // [4][2]
    unsigned* shu = reinterpret_cast<unsigned*>(red_i + 8);       // [4]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int MT = p.M * p.T;
    for (int c = tid; c < p.C; c += OI_THREADS) seen[c] = 0;
    for (int w = tid; w < W; w += OI_THREADS) labset[w] = 0u;
    for (int k = tid; k < MT; k += OI_THREADS) gscore[k] = 0.f;
    __syncthreads();
    for (int j = tid; j < p.M; j += OI_THREADS) {
        const long long at = (long long)b * p.M + j;
        const long long c1 = p.gt_cls[at];
        const int cls = (c1 >= 1 && c1 <= p.C) ? (int)(c1 - 1) : -1;
        gcls[j] = cls;
        gflag[j] = ((p.gt_difficult && p.gt_difficult[at]) ? OI_DIFFICULT : 0) | ((p.gt_group_of && p.gt_group_of[at]) ? OI_GROUP_OF : 0);
        taken[j] = 0;
        if (cls >= 0 && p.labeled_cls) atomicOr(&labset[cls >> 5], 1u << (cls & 31));
    }
    if (p.labeled_cls)
        for (int k = tid; k < p.K; k += OI_THREADS) {
            const long long c1 = p.labeled_cls[(long long)b * p.K + k];
            if (c1 >= 1 && c1 <= p.C) atomicOr(&labset[(int)(c1 - 1) >> 5], 1u << ((int)(c1 - 1) & 31));
        }
    __syncthreads();
    for (int j = tid; j < p.M; j += OI_THREADS) {                 // the counters, by integer atomics (order independent)
        const int c = gcls[j];
        if (c < 0) continue;
        const int f = gflag[j];
        if (f == 0) atomicAdd(p.n_plain + c, 1);
        if (f == OI_GROUP_OF) atomicAdd(p.n_group + c, 1);
        bool first = true;
        for (int q = 0; q < j; ++q) first = first && gcls[q] != c;
        if (first) atomicAdd(p.gt_imgs + c, 1);
    }
    const int n = min(p.det_count[b], p.max_det);
    int kept = 0, nans = 0;                                       // thread 0's
    for (int i = 0; i < p.max_det; ++i) {
        unsigned* out = p.flags + (long long)b * p.max_det + i;
        if (i >= n) { if (tid == 0) *out = OI_INVALID; continue; }
        const float* d = p.det + ((long long)b * p.max_det + i) * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4];
        const int c = (int)d[5] - 1;
        if (score != score) ++nans;
        bool ok = y1 < y2 && x1 < x2 && c >= 0 && c < p.C && score == score;
        if (ok && p.labeled_cls) ok = (labset[c >> 5] >> (c & 31)) & 1u;
        if (!ok) { if (tid == 0) *out = OI_INVALID; continue; }   // the same for the whole workgroup
        const EmDet dd = em_det(x1, y1, x2, y2);
        float b1 = -1.f, bg = -1.f, ba = -1.f;                    // best IoU of a plain box, of a group-of box, best IoA of a group-of box
        int j1 = EM_NO_BOX, ja = EM_NO_BOX;
        for (int j = tid; j < p.M; j += OI_THREADS) {             // ascending j: the first maximum is kept
            if (gcls[j] != c) continue;
            const float* g = p.gt_boxes + ((long long)b * p.M + j) * 4;        // yxyx
            const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
            const float v = em_iou(dd, g0, g1, g2, g3);
            if (gflag[j] & OI_GROUP_OF) {
                if (v > bg) bg = v;
                const float a = em_iou_crowd(dd, g0, g1, g2, g3);
                if (a > ba) { ba = a; ja = j; }
            } else if (v > b1) { b1 = v; j1 = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float o1 = __shfl_xor(b1, o, 64), oa = __shfl_xor(ba, o, 64);
            const int q1 = __shfl_xor(j1, o, 64), qa = __shfl_xor(ja, o, 64);
            bg = fmaxf(bg, __shfl_xor(bg, o, 64));
            if (o1 > b1 || (o1 == b1 && q1 < j1)) { b1 = o1; j1 = q1; }
            if (oa > ba || (oa == ba && qa < ja)) { ba = oa; ja = qa; }
        }
        if (lane == 0) { red_v[3 * wave] = b1; red_v[3 * wave + 1] = bg; red_v[3 * wave + 2] = ba; red_i[2 * wave] = j1; red_i[2 * wave + 1] = ja; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < OI_THREADS / 64; ++w) {
                const float o1 = red_v[3 * w], oa = red_v[3 * w + 2];
                const int q1 = red_i[2 * w], qa = red_i[2 * w + 1];
                bg = fmaxf(bg, red_v[3 * w + 1]);
                if (o1 > b1 || (o1 == b1 && q1 < j1)) { b1 = o1; j1 = q1; }
                if (oa > ba || (oa == ba && qa < ja)) { ba = oa; ja = qa; }
            }
            const bool has1 = j1 != EM_NO_BOX, hasg = ja != EM_NO_BOX;
            const float ball = fmaxf(b1, bg);                     // CorLoc: every box of the class, by IoU
            unsigned reach1 = 0, reacha = 0, reachall = 0;
            for (int t = 0; t < p.T; ++t) {
                reach1 |= (has1 && b1 >= p.thr[t] ? 1u : 0u) << t;
                reacha |= (hasg && ba >= p.thr[t] ? 1u : 0u) << t;
                reachall |= ((has1 || hasg) && ball >= p.thr[t] ? 1u : 0u) << t;
            }
            unsigned tp = 0, ign = 0;
            if (has1 && j1 < p.M) {
                if (gflag[j1] & OI_DIFFICULT) ign = reach1;
                else { tp = reach1 & ~(unsigned)taken[j1]; taken[j1] |= (int)reach1; }
            }
            const unsigned absorbed = reacha & ~(tp | ign);
            if (absorbed && ja < p.M)
                for (int t = 0; t < p.T; ++t)
                    if ((absorbed >> t) & 1u) {
                        float* g = gscore + (long long)ja * p.T + t;
                        if (score > *g) *g = score;
                    }
            *out = tp | ((ign | absorbed) << 16);
            ++kept;
            if (!seen[c]) {                                       // top-scoring detection of class c
                seen[c] = 1;
                for (int t = 0; t < p.T; ++t)
                    if ((reachall >> t) & 1u) atomicAdd(p.correct + (long long)t * p.C + c, 1);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    // the image's virtual entries: slot j T + t
    const unsigned all = (1u << p.T) - 1u;
    unsigned emitted = 0;
    for (int k = tid; k < MT; k += OI_THREADS) {
        const int j = k / p.T, t = k - j * p.T;
        const float s = gscore[k];
        const bool e = p.emit && gcls[j] >= 0 && (gflag[j] & OI_GROUP_OF) && s > 0.f;
        p.vscore[(long long)b * MT + k] = e ? s : 0.f;
        p.vflags[(long long)b * MT + k] = e ? ((1u << t) | ((all & ~(1u << t)) << 16) | OI_GROUP) : OI_INVALID;
        emitted += e ? 1u : 0u;
    }
    emitted = ev_block_sum<unsigned>(emitted, shu, tid);
    if (tid == 0) { p.kept[b] = kept + (int)emitted; p.kept[p.B + b] = nans; }
}

// ---- append: ev_append_write_kernel of eval_sorted.h with the image's virtual slots behind its detection slots -------------------
struct OiAppend {
    const float* det; const unsigned* flags; const long long* gt_cls; const float* vscore; const unsigned* vflags; const int* kept;
    int B, max_det, M, T;
    float* scores; int* classes; unsigned* out_flags; unsigned capacity; unsigned* state;
};

__global__ __launch_bounds__(OI_THREADS) void oi_append_write_kernel(OiAppend a) {
    __shared__ unsigned shu[EV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned before = 0;
    for (int k = tid; k < b; k += OI_THREADS) before += (unsigned)a.kept[k];
    unsigned pos = fo_min(a.state[0], a.capacity) + ev_block_sum<unsigned>(before, shu, tid);
    for (int i0 = 0; i0 < a.max_det; i0 += OI_THREADS) {
        const int i = i0 + tid;
        const long long slot = (long long)b * a.max_det + i;
        unsigned word = 0;
        bool keep = false;
        if (i < a.max_det) { word = a.flags[slot]; keep = !(word & OI_INVALID); }
        unsigned total;
        const unsigned p = pos + fo_block_excl_scan(keep ? 1u : 0u, shu, tid, &total);
        if (keep && p < a.capacity) {                                     // beyond the capacity: counted by the cursor launch
            float v = a.det[slot * 6 + 4];
            if (v == 0.f) v = 0.f;                                        // -0.0 is stored as +0.0: the two tie
            a.scores[p] = v;
            a.classes[p] = (int)a.det[slot * 6 + 5] - 1;
            a.out_flags[p] = word;
        }
        pos += total;
    }
    const int MT = a.M * a.T;
    for (int k0 = 0; k0 < MT; k0 += OI_THREADS) {
        const int k = k0 + tid;
        unsigned word = 0;
        bool keep = false;
        if (k < MT) { word = a.vflags[(long long)b * MT + k]; keep = !(word & OI_INVALID); }
        unsigned total;
        const unsigned p = pos + fo_block_excl_scan(keep ? 1u : 0u, shu, tid, &total);
        if (keep && p < a.capacity) {
            a.scores[p] = a.vscore[(long long)b * MT + k];
            a.classes[p] = (int)a.gt_cls[(long long)b * a.M + k / a.T] - 1;
            a.out_flags[p] = word;
        }
        pos += total;
    }
}

// ---- sort: by (class, score descending), the flag word as payload; then, for the pooled AP, the sorted entries again by score ----
struct OiItem { u64 key; unsigned val; };
struct OiSort : EvSort { typedef OiItem Item; const unsigned* flags; };
DEV u64 rs_key(const OiSort& s, unsigned, unsigned i) {
    return ev_key(s, i, [&s](unsigned k) { return !(s.flags[k] & OI_INVALID); });
}
DEV OiItem rs_load(const OiSort& s, unsigned, unsigned i) { return OiItem{rs_key(s, 0, i), s.first ? s.flags[i] : s.src_v[i]}; }
DEV void rs_store(const OiSort& s, unsigned, unsigned p, const OiItem& e) { s.dst_k[p] = e.key; s.dst_v[p] = e.val; }

DEV double oi_num_gt(int n_plain, int n_group, double w) { return (double)n_plain + w * (double)n_group; }

// pk, pv: the class-sorted keys and flag words.  The key keeps the score part; its class becomes 0, or 1 for an entry that is not
// valid or whose class has no instances: the stable sort leaves equal scores in (class, arrival) order.
struct OiPoolSort : EvSort {
    typedef OiItem Item;
    const u64* pk; const unsigned* pv; const int* n_plain; const int* n_group; double w; int num_classes;
};
DEV u64 rs_key(const OiPoolSort& s, unsigned, unsigned i) {
    if (!s.first) return s.src_k[i];
    const u64 k = s.pk[i];
    const unsigned c = (unsigned)(k >> 32);
    const bool ok = c < (unsigned)s.num_classes && oi_num_gt(s.n_plain[c], s.n_group[c], s.w) > 0.0;
    return ((u64)(ok ? 0u : 1u) << 32) | (k & 0xFFFFFFFFull);
}
DEV OiItem rs_load(const OiPoolSort& s, unsigned, unsigned i) { return OiItem{rs_key(s, 0, i), s.first ? s.pv[i] : s.src_v[i]}; }
DEV void rs_store(const OiPoolSort& s, unsigned, unsigned p, const OiItem& e) { s.dst_k[p] = e.key; s.dst_v[p] = e.val; }

// ---- average precision -----------------------------------------------------------------------------------------------------------
// All threads of the workgroup: the weighted VOC AP at threshold t of the sorted entries [s, e) (one segment), s < e, num_gt > 0.
// The totals first, then the chunks from the last to the first, as es_ap_kernel: rank, a and g by integer scans.
DEV double oi_ap_segment(const unsigned* flags, unsigned s, unsigned e, int t, double w, double num_gt, unsigned* shu, double* shd, int tid) {
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    unsigned rem_ni = 0, rem_a = 0, rem_g = 0;
    for (unsigned i0 = s; i0 < e; i0 += OI_THREADS * 256) {               // a thread adds up to 256 entries before the sums are unpacked
        unsigned tot = 0, tg = 0;
        unsigned i = i0 + tid;
        for (unsigned r = 0; r < 256 && i < e; ++r, i += OI_THREADS) {
            const unsigned f = flags[i];
            const bool tp = f & tp_bit, grp = f & OI_GROUP;
            tot += ((f & ig_bit) ? 0u : 1u) + ((tp && !grp) ? 0x10000u : 0u);
            tg += (tp && grp) ? 1u : 0u;
        }
        rem_ni += ev_block_sum<unsigned>(tot & 0xFFFFu, shu, tid);
        rem_a += ev_block_sum<unsigned>(tot >> 16, shu, tid);
        rem_g += ev_block_sum<unsigned>(tg, shu, tid);
    }
    double acc = 0.0, carry = 0.0;                                        // carry: largest precision of the chunks behind this one
    const unsigned nchunks = (e - s + EV_AP_CHUNK - 1) / EV_AP_CHUNK;
    for (unsigned q = nchunks; q-- > 0;) {
        const unsigned i0 = s + q * EV_AP_CHUNK + (unsigned)tid * EV_AP_ITEMS;
        unsigned f[EV_AP_ITEMS], cnt = 0, cg = 0;
#pragma unroll
        for (int r = 0; r < EV_AP_ITEMS; ++r) {
            f[r] = i0 + r < e ? flags[i0 + r] : ig_bit;                    // beyond the segment: ignored
            const bool tp = f[r] & tp_bit, grp = f[r] & OI_GROUP;
            cnt += ((f[r] & ig_bit) ? 0u : 1u) + ((tp && !grp) ? 0x10000u : 0u);
            cg += (tp && grp) ? 1u : 0u;
        }
        unsigned total, total_g;
        const unsigned ex = fo_block_excl_scan(cnt, shu, tid, &total);
        const unsigned exg = fo_block_excl_scan(cg, shu, tid, &total_g);
        rem_ni -= total & 0xFFFFu; rem_a -= total >> 16; rem_g -= total_g;      // now: the counts in front of this chunk
        unsigned rank = rem_ni + (ex & 0xFFFFu), a = rem_a + (ex >> 16), g = rem_g + exg;
        double prec[EV_AP_ITEMS], step[EV_AP_ITEMS];
#pragma unroll
        for (int r = 0; r < EV_AP_ITEMS; ++r) {
            const bool ni = !(f[r] & ig_bit), tp = f[r] & tp_bit, grp = f[r] & OI_GROUP;
            const double before = (double)a + w * (double)g;
            rank += ni ? 1u : 0u; a += (tp && !grp) ? 1u : 0u; g += (tp && grp) ? 1u : 0u;
            const double ctp = (double)a + w * (double)g;
            prec[r] = ni ? ctp / (ctp + (double)(rank - a - g)) : 0.0;
            step[r] = tp ? ctp / num_gt - before / num_gt : 0.0;
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
    return acc;
}

struct OiAp {
    const u64* keys; const unsigned* flags;                               // sorted by (class, score)
    const u64* pool_keys; const unsigned* pool_flags;                     // sorted by score; null: no pooled AP
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C; double w;
    const int* n_plain; const int* n_group; const int* gt_imgs; const int* correct;
    u64* result;
};

DEV double* oi_res_ap(const OiAp& a) { return reinterpret_cast<double*>(a.result + OI_RESULT_HEAD); }
DEV double* oi_res_pooled(const OiAp& a) { return oi_res_ap(a) + (long long)a.T * a.C; }
DEV long long* oi_res_counts(const OiAp& a) { return reinterpret_cast<long long*>(oi_res_pooled(a) + a.T); }

// workgroup (c, t): AP of class c at threshold t, and the (c, t) entries of the result block
__global__ __launch_bounds__(OI_THREADS) void oi_ap_kernel(OiAp a) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ double shd[EV_WAVES];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const unsigned n = ev_live(a.state, a.n_host, a.capacity);
    const unsigned s = ev_class_begin(a.keys, n, c), e = ev_class_begin(a.keys, n, c + 1);
    const double num_gt = oi_num_gt(a.n_plain[c], a.n_group[c], a.w);
    double acc = 0.0;
    if (num_gt > 0.0 && e > s) acc = oi_ap_segment(a.flags, s, e, t, a.w, num_gt, shu, shd, tid);      // the same for the whole workgroup
    if (tid != 0) return;
    long long* cnt = oi_res_counts(a);
    oi_res_ap(a)[(long long)t * a.C + c] = num_gt > 0.0 ? acc : __builtin_nan("");
    cnt[3ll * a.C + (long long)t * a.C + c] = a.correct[(long long)t * a.C + c];
    if (t == 0) { cnt[c] = a.n_plain[c]; cnt[a.C + c] = a.n_group[c]; cnt[2ll * a.C + c] = a.gt_imgs[c]; }
    if (t == 0 && c == 0) {
        u64* res = a.result;
        res[0] = n; res[1] = a.state ? a.state[1] : 0; res[2] = a.state ? a.state[2] : 0; res[3] = (u64)a.T; res[4] = (u64)a.C;
        res[5] = a.pool_keys ? 1 : 0; res[6] = 0; res[7] = 0;
    }
}

// workgroup t: the pooled AP at threshold t over the entries of the classes with instances (NaN: not asked for, or no instances)
__global__ __launch_bounds__(OI_THREADS) void oi_pooled_ap_kernel(OiAp a) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ double shd[EV_WAVES];
    __shared__ u64 shl[EV_WAVES];
    const int t = blockIdx.x, tid = threadIdx.x;
    double out = __builtin_nan("");
    if (a.pool_keys) {                                                    // the same for the whole workgroup
        u64 np = 0, ng = 0;
        for (int c = tid; c < a.C; c += OI_THREADS)
            if (oi_num_gt(a.n_plain[c], a.n_group[c], a.w) > 0.0) { np += (u64)a.n_plain[c]; ng += (u64)a.n_group[c]; }
        np = ev_block_sum<u64>(np, shl, tid);
        ng = ev_block_sum<u64>(ng, shl, tid);
        const double num_gt = (double)np + a.w * (double)ng;
        const unsigned n = ev_live(a.state, a.n_host, a.capacity);
        const unsigned e = ev_class_begin(a.pool_keys, n, 1);
        if (num_gt > 0.0) out = e > 0 ? oi_ap_segment(a.pool_flags, 0, e, t, a.w, num_gt, shu, shd, tid) : 0.0;
    }
    if (tid == 0) oi_res_pooled(a)[t] = out;
}

// ---- workspace layout (host): the class sort's buffers, then the pooled sort's ---------------------------------------------------------
bool oi_layout(long long capacity, int C, int pooled, EvLayout* L, EvLayout* P, long long* total) {
    if (!ev_layout(capacity, C, 0, 0, L) || !ev_layout(capacity, 1, 0, 0, P)) return false;
    *total = L->total + (pooled ? P->total : 0);
    return true;
}

bool oi_weight_ok(double w) { return w >= 0.0 && w <= 1.7976931348623157e308; }      // not negative, not NaN, finite

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_openimages_match_lds_bytes(int M, int num_classes, int num_thresholds) {
    return oi_match_lds(M, num_classes, num_thresholds);
}

extern "C" int effdet_openimages_match(void* stream, const float* det, const int* det_count, const float* gt_boxes,
                                       const long long* gt_cls, const unsigned char* gt_difficult, const unsigned char* gt_group_of,
                                       const long long* labeled_cls, int K, int B, int max_det, int M, int num_classes,
                                       const float* thresholds, int num_thresholds, int emit_virtual, unsigned int* flags,
                                       float* vscore, unsigned int* vflags, int* kept, int* n_plain, int* n_group, int* gt_imgs,
                                       int* correct_imgs) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !flags || !vscore || !vflags || !kept || !n_plain || !n_group ||
        !gt_imgs || !correct_imgs)
        return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, OI_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15, ascending, no NaN
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if ((long long)B * M * num_thresholds > EM_MAX_N) return EFFDET_EINVAL;      // B M num_thresholds virtual slots exceed 2^24
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    if (labeled_cls && K < 0) return EFFDET_EINVAL;      // a label list of negative length
    const long long sh = oi_match_lds(M, num_classes, num_thresholds);
    if (sh < 0 || sh > 64 * 1024) return EFFDET_EINVAL;      // (num_classes + ceil(num_classes / 32) + (3 + num_thresholds) M + 24) words exceed 64 KiB of LDS
    OiMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_difficult = gt_difficult;
    a.gt_group_of = gt_group_of; a.labeled_cls = labeled_cls;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds; a.K = labeled_cls ? K : 0;
    a.emit = emit_virtual ? 1 : 0;
    for (int t = 0; t < OI_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.flags = flags; a.vscore = vscore; a.vflags = vflags; a.kept = kept; a.n_plain = n_plain; a.n_group = n_group;
    a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    hipLaunchKernelGGL(oi_match_kernel, dim3(B), dim3(OI_THREADS), (size_t)sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_openimages_append(void* stream, const float* det, const unsigned int* flags, const long long* gt_cls,
                                        const float* vscore, const unsigned int* vflags, const int* kept, int B, int max_det, int M,
                                        int num_thresholds, float* scores, int* classes, unsigned int* out_flags, long long capacity,
                                        unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !gt_cls || !vscore || !vflags || !kept || !scores || !classes || !out_flags || !state)
        return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (num_thresholds < 1 || num_thresholds > OI_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15
    if ((long long)B * M * num_thresholds > EM_MAX_N) return EFFDET_EINVAL;      // B M num_thresholds virtual slots exceed 2^24
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    const OiAppend a{det, flags, gt_cls, vscore, vflags, kept, B, max_det, M, num_thresholds, scores, classes, out_flags,
                     (unsigned)capacity, state};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(oi_append_write_kernel, dim3(B), dim3(OI_THREADS), 0, st, a);
    hipLaunchKernelGGL(ev_append_cursor_kernel, dim3(1), dim3(EV_THREADS), 0, st, EvCursor{kept, B, (unsigned)capacity, state});
    return effdet_check_launch();
}

extern "C" long long effdet_openimages_sorted_workspace_bytes(long long capacity, int num_classes, int pooled) {
    EvLayout L, P;
    long long total;
    return oi_layout(capacity, num_classes, pooled, &L, &P, &total) ? total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_openimages_sorted_offset(long long capacity, int num_classes, int which) {
    EvLayout L, P;
    long long total;
    if (which < 0 || which > 3 || !oi_layout(capacity, num_classes, 1, &L, &P, &total)) return EFFDET_EINVAL;
    if (which < 2) return which == 0 ? L.keys[ev_last(L)] : L.vals[ev_last(L)];
    return L.total + (which == 2 ? P.keys[ev_last(P)] : P.vals[ev_last(P)]);
}

extern "C" long long effdet_openimages_sorted_result_bytes(int num_thresholds, int num_classes) {
    if (num_thresholds < 1 || num_thresholds > OI_MAX_T || !em_classes_ok(num_classes)) return EFFDET_EINVAL;
    return 8ll * (OI_RESULT_HEAD + 2ll * num_thresholds * num_classes + num_thresholds + 3ll * num_classes);
}

extern "C" int effdet_openimages_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                        long long capacity, long long n, const unsigned int* state, int num_thresholds,
                                        int num_classes, double group_of_weight, int pooled, const int* n_plain, const int* n_group,
                                        const int* gt_imgs, const int* correct_imgs, void* workspace, long long workspace_bytes,
                                        void* result) {
    EFFDET_ENTER();
    if (!scores || !classes || !flags || !n_plain || !n_group || !gt_imgs || !correct_imgs || !workspace || !result)
        return EFFDET_EINVAL;      // null pointer
    if (n < 0 && !state) return EFFDET_EINVAL;      // n < 0 takes the count from `state`, which is null
    if (num_thresholds < 1 || num_thresholds > OI_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    if (!oi_weight_ok(group_of_weight)) return EFFDET_EINVAL;      // group_of_weight must be finite and not negative
    EvLayout L, P;
    long long total;
    if (!oi_layout(capacity, num_classes, pooled, &L, &P, &total)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    if (n > capacity) return EFFDET_EINVAL;      // n exceeds the capacity
    if (workspace_bytes < total) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(result) % 8)
        return EFFDET_EINVAL;      // workspace and result must be 8-byte aligned
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long n_host = n < 0 ? -1 : n;
    OiSort s;
    s.flags = flags;
    ev_sort(st, s, scores, classes, state, n_host, capacity, num_classes, ws, L, [](OiSort&, int) {});
    const int last = ev_last(L);
    OiAp a;
    a.keys = reinterpret_cast<const u64*>(ws + L.keys[last]); a.flags = reinterpret_cast<const unsigned*>(ws + L.vals[last]);
    a.pool_keys = nullptr; a.pool_flags = nullptr;
    a.state = state; a.n_host = n_host; a.capacity = (unsigned)capacity;
    a.T = num_thresholds; a.C = num_classes; a.w = group_of_weight;
    a.n_plain = n_plain; a.n_group = n_group; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    a.result = reinterpret_cast<u64*>(result);
    if (pooled) {
        char* pws = ws + L.total;
        OiPoolSort q;
        q.pk = a.keys; q.pv = a.flags; q.n_plain = n_plain; q.n_group = n_group; q.w = group_of_weight; q.num_classes = num_classes;
        ev_sort(st, q, scores, classes, state, n_host, capacity, 1, pws, P, [](OiPoolSort&, int) {});
        a.pool_keys = reinterpret_cast<const u64*>(pws + P.keys[ev_last(P)]);
        a.pool_flags = reinterpret_cast<const unsigned*>(pws + P.vals[ev_last(P)]);
    }
    hipLaunchKernelGGL(oi_ap_kernel, dim3((unsigned)num_classes, (unsigned)num_thresholds), dim3(OI_THREADS), 0, st, a);
    hipLaunchKernelGGL(oi_pooled_ap_kernel, dim3((unsigned)num_thresholds), dim3(OI_THREADS), 0, st, a);
    return effdet_check_launch();
}
