// COCO-protocol detection evaluation on the device: COCOeval.evaluateImg / accumulate / summarize for iouType 'bbox',
// for a whole validation set, at T <= 15 IoU thresholds, A <= 4 area ranges and Mx <= 4 `max_dets` in one matching pass and one sort.
// Compiled with -ffp-contract=off: the IoU rounds like eval_match.h's separate float32 operations, every float64 term of precision
// and recall is one division or one addition, one rounding each.
//
// Definitions (restated in tests/_coco_eval_ref.py).  Per image: det [max_det][6] rows x1, y1, x2, y2, score, 1-based class in
// descending score order, count valid rows; ground truth boxes yxyx with a 1-based class (<= 0: padding), a crowd byte and an area
// (null: the float32 box area (y2 - y1) * (x2 - x1); COCO's annotation `area` is not the box area).
//   dropped   a slot beyond the count, with a degenerate box (!(y1 < y2 && x1 < x2)), a class outside 1..C, a NaN score, a score
//             < min_score, or whose 0-based rank among the kept slots of its class in the image is >= max_dets[-1] (pycocotools
//             truncates before it matches).  The rank travels with the slot.
//   IoU       em_iou in float32; against a crowd box the same intersection over the detection's area (em_iou_crowd).
//   ignore    box g is ignored at area range a iff it is crowd, or area_g < lo_a, or area_g > hi_a.
//   matching  per (t, a), detections in slot order: among the boxes of the detection's class first those not ignored at a and not
//             taken at (t, a): the largest IoU >= thr_t, the LAST index on equal IoU.  Only if there is none, the ignored boxes
//             (a crowd box whether taken or not, another ignored box only if not taken at (t, a)), by the same rule.  Matched to
//             a box that is not ignored: true positive, the box is taken at (t, a).  Matched to an ignored box: the detection is
//             ignored at (t, a); a box that is not crowd is taken.  Unmatched: ignored iff the detection's own box area lies
//             outside [lo_a, hi_a], otherwise a false positive.
//   output    A flag words per slot (bit t: true positive, bit 16 + t: ignored, bit 31: dropped) and the rank (-1: dropped).
//   npig      [C][A]: the boxes of class c not ignored at a (integer atomics: order independent).
//   AP / AR   per (t, c, a, m), over the class's entries in (score descending, arrival order) with rank < max_dets[m] that are not
//             ignored at (t, a): cumulative tp and fp; rc = tp / npig; pr = tp / ((fp + tp) + 2^-52) in float64; pr made
//             non-increasing from the right; q[r] = pr[first i with rc[i] >= rec_thr[r]], 0 if there is none; AP = (q[0] + q[1] +
//             ... in ascending r, one addition each) / R; AR = the last rc, 0 without entries; both NaN when npig[c][a] = 0.
//
// Kernels
//   match    one workgroup per image, the detections walked serially.  The image's boxes, classes and ignore bits are staged in
//            LDS once.  Per kept detection the workgroup writes the IoU row against the boxes of its class into LDS; then the
//            lanes of wave 0 each own one (t, a) pair (T A <= 60) and walk that row, keeping the best free box and the best
//            ignored box at once.  `taken` is one 64-bit word per box (bit t A + a), set by a 64-bit LDS atomic OR because two
//            lanes may take the same box; a lane reads only its own bit, so the pairs never wait for each other.  Two ballots
//            turn the lanes' verdicts into the A flag words.
//   append   ev_append of eval_sorted.h: positions from the images' kept counts and a cursor on the device; the payload of an
//            entry beside (score, class) is its A words and its rank.
//   sort     ev_sort over the 48-bit (class, score descending) key with the ENTRY INDEX as payload, so the scatter kernel's
//            registers hold one payload word whatever A is; one gather launch then lays words and ranks out in sorted order.
//   AP       one workgroup per (c, t, a, m) - C T A Mx of them (9600 for COCO), each over a segment of n / C entries: more
//            workgroups than the device has wave slots and no serial loop over pairs inside one.  The chunks of 2048 go from the
//            back: an integer scan gives rank and cumulative tp, a reverse max-scan carried from chunk to chunk the envelope.
//            Thread r first finds k_r, the smallest k with k / npig >= rec_thr[r] (k_r = 0: the first entry); the thread that holds
//            the true positive with cumulative count k writes q[r] for every r with k_r = k (a binary search over the ascending
//            k_r), so each q[r] has one writer.  Thread 0 adds q in ascending r.  No floating-point atomics.
// Launch boundaries are the only synchronisation between workgroups; every loop has a trip count known at its entry; every index
// is compared with its extent before a store; the live count is read from the device cursor and grids are sized by the capacity.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"
#include "eval_match.h"
#include "eval_sorted.h"

namespace {

constexpr int CC_THREADS = EV_THREADS;
constexpr int CC_MAX_MX = 4, CC_MAX_R = 256;
constexpr int CC_RESULT_HEAD = 8;                                 // 8-byte words before the AP array
constexpr int CC_NO_K = 0x7fffffff;                               // k_r of a recall threshold that no count reaches

// ---- matching --------------------------------------------------------------------------------------------------------------------
struct CcMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls; const unsigned char* gt_crowd;
    const float* gt_area;
    int B, max_det, M, C, T, A, max_rank; float min_score; float thr[EM_MAX_T]; float lo[EM_MAX_A], hi[EM_MAX_A];
    unsigned* flags; int* rank; int* kept; int* npig;
};

size_t cc_match_lds(int M, int C) { return 40 * (size_t)M + 4 * (size_t)C; }

__global__ __launch_bounds__(CC_THREADS) void cc_match_kernel(CcMatch p) {
    extern __shared__ double cc_lds[];
    u64* taken = reinterpret_cast<u64*>(cc_lds);                  // [M] bit t A + a: taken at (t, a)
    float* box = reinterpret_cast<float*>(taken + p.M);           // [M][4] yxyx
    float* iou = box + 4 * p.M;                                   // [M] the detection's row
    int* gcls = reinterpret_cast<int*>(iou + p.M);                // [M] 0-based class or -1
    int* gmeta = gcls + p.M;                                      // [M] bit a: ignored at a, EM_ROW_CROWD
    int* rmeta = gmeta + p.M;                                     // [M] gmeta | EM_ROW_OF_CLASS for the boxes of the detection's class, else 0
    int* seen = rmeta + p.M;                                      // [C] kept detections of the class so far
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < p.C; c += CC_THREADS) seen[c] = 0;
    for (int j = tid; j < p.M; j += CC_THREADS) {
        const long long at = (long long)b * p.M + j;
        const long long c1 = p.gt_cls[at];
        const int cls = (c1 >= 1 && c1 <= p.C) ? (int)(c1 - 1) : -1;
        const float* g = p.gt_boxes + at * 4;
        const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
        box[4 * j] = g0; box[4 * j + 1] = g1; box[4 * j + 2] = g2; box[4 * j + 3] = g3;
        const bool crowd = p.gt_crowd && p.gt_crowd[at];
        const float area = p.gt_area ? p.gt_area[at] : (g2 - g0) * (g3 - g1);
        int meta = crowd ? EM_ROW_CROWD : 0;
#pragma unroll
        for (int a = 0; a < EM_MAX_A; ++a) {
            if (a >= p.A) continue;
            const bool ig = crowd || area < p.lo[a] || area > p.hi[a];
            meta |= (ig ? 1 : 0) << a;
            if (cls >= 0 && !ig) atomicAdd(p.npig + (long long)cls * p.A + a, 1);
        }
        gcls[j] = cls; gmeta[j] = meta; taken[j] = 0;
    }
    // lane `pair` of wave 0 owns (t, a)
    const int pair = tid & 63;
    const bool active = tid < 64 && pair < p.T * p.A;
    const int my_t = pair / p.A, my_a = pair % p.A;
    float my_thr = 0.f, my_lo = 0.f, my_hi = 0.f;
#pragma unroll
    for (int t = 0; t < EM_MAX_T; ++t) if (t == my_t) my_thr = p.thr[t];
#pragma unroll
    for (int a = 0; a < EM_MAX_A; ++a) if (a == my_a) { my_lo = p.lo[a]; my_hi = p.hi[a]; }
    __syncthreads();
    const int n = min(p.det_count[b], p.max_det);
    int kept = 0, nans = 0;                          // thread 0's
    for (int i = 0; i < p.max_det; ++i) {
        const long long slot = (long long)b * p.max_det + i;
        const float* d = p.det + slot * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4], cf = d[5];
        const int c = (cf >= 1.f && cf < (float)(p.C + 1)) ? (int)cf - 1 : -1;
        if (i < n && score != score) ++nans;
        bool ok = i < n && y1 < y2 && x1 < x2 && c >= 0 && score == score && !(score < p.min_score);
        const int rk = ok ? seen[c] : 0;             // written by thread 0 before the barrier that ended the last kept round
        ok = ok && rk < p.max_rank;
        if (!ok) {                                   // the same for the whole workgroup
            if (tid < p.A) p.flags[slot * p.A + tid] = EM_DROPPED;
            if (tid == 0) p.rank[slot] = -1;
            continue;
        }
        const EmDet dd = em_det(x1, y1, x2, y2);
        for (int j = tid; j < p.M; j += CC_THREADS) {
            int m = 0;
            if (gcls[j] == c) {
                m = gmeta[j] | EM_ROW_OF_CLASS;
                const float* g = box + 4 * j;
                iou[j] = (m & EM_ROW_CROWD) ? em_iou_crowd(dd, g[0], g[1], g[2], g[3]) : em_iou(dd, g[0], g[1], g[2], g[3]);
            }
            rmeta[j] = m;
        }
        __syncthreads();
        if (tid < 64) {
            int b1 = -1, b2 = -1;                    // the best box not ignored / ignored at my_a
            if (active) em_walk_row(rmeta, taken, iou, p.M, pair, my_a, my_thr, &b1, &b2);
            const int bj = b1 >= 0 ? b1 : b2;
            const bool tp = active && b1 >= 0;
            const bool ign = active && b1 < 0 && (b2 >= 0 || dd.area < my_lo || dd.area > my_hi);
            if (active && bj >= 0 && !(rmeta[bj] & EM_ROW_CROWD)) atomicOr(&taken[bj], (u64)(1ull << pair));
            const u64 tpm = __ballot(tp), igm = __ballot(ign);
            if (tid < p.A) {
                unsigned w = 0;
                for (int t = 0; t < p.T; ++t) {
                    const int bit = t * p.A + tid;
                    w |= (unsigned)((tpm >> bit) & 1ull) << t;
                    w |= (unsigned)((igm >> bit) & 1ull) << (16 + t);
                }
                p.flags[slot * p.A + tid] = w;
            }
            if (tid == 0) { p.rank[slot] = rk; seen[c] = rk + 1; ++kept; }
        }
        __syncthreads();                             // the row, `taken` and `seen` are settled for the next detection
    }
    if (tid == 0 && p.kept) { p.kept[b] = kept; p.kept[p.B + b] = nans; }
}

// ---- append: the A flag words and the rank travel with (score, class) -------------------------------------------------------------
struct CcAppend : EvAppend { const unsigned* flags; const int* rank; int A; unsigned* words; int* ranks; };
DEV bool ev_keep(const CcAppend& a, long long slot, unsigned* word) { *word = a.flags[slot * a.A]; return !(*word & EM_DROPPED); }
DEV void ev_store(const CcAppend& a, long long slot, unsigned p, unsigned) {      // the A words are read again, as they always were
    for (int w = 0; w < a.A; ++w) a.words[(long long)p * a.A + w] = a.flags[slot * a.A + w];
    a.ranks[p] = a.rank[slot];
}

// ---- sort: the pass descriptor of radix_sort.h; the payload is the entry's index --------------------------------------------------
struct CcItem { u64 key; unsigned val; };
struct CcSort : EvSort { typedef CcItem Item; };
DEV u64 rs_key(const CcSort& s, unsigned, unsigned i) { return ev_key(s, i, [](unsigned) { return true; }); }
DEV CcItem rs_load(const CcSort& s, unsigned, unsigned i) {
    CcItem e;
    e.key = rs_key(s, 0, i);
    e.val = s.first ? i : s.src_v[i];
    return e;
}
DEV void rs_store(const CcSort& s, unsigned, unsigned p, const CcItem& e) { s.dst_k[p] = e.key; s.dst_v[p] = e.val; }

struct CcGather {
    const unsigned* index; const unsigned* words; const int* ranks; const unsigned* cursor; long long n_host; unsigned capacity; int A;
    unsigned* out_words; int* out_ranks;
};
// thread i: the words and the rank of the entry at sorted position i
__global__ __launch_bounds__(CC_THREADS) void cc_gather_kernel(CcGather g) {
    const unsigned i = blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= ev_live(g.cursor, g.n_host, g.capacity)) return;
    const unsigned src = g.index[i];
    if (src >= g.capacity) return;
    for (int w = 0; w < g.A; ++w) g.out_words[(long long)i * g.A + w] = g.words[(long long)src * g.A + w];
    g.out_ranks[i] = g.ranks[src];
}

// ---- average precision and recall ------------------------------------------------------------------------------------------------
struct CcAp {
    const u64* keys; const unsigned* words; const int* ranks;             // sorted
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C, A, Mx, R; int maxdet[CC_MAX_MX];
    const double* rec_thr; const int* npig;
    u64* result; double* precision;
};

// workgroup (c, (t, a, m)): bit 0 of an entry = it counts (rank < max_dets[m], not ignored at (t, a)), bit 1 = true positive
__global__ __launch_bounds__(CC_THREADS) void cc_ap_kernel(CcAp p) {
    __shared__ unsigned shu[EV_WAVES];
    __shared__ double shd[EV_WAVES];
    __shared__ int kr[CC_MAX_R];
    __shared__ double q[CC_MAX_R];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int m = blockIdx.y % p.Mx, a = (blockIdx.y / p.Mx) % p.A, t = blockIdx.y / (p.Mx * p.A);
    int md = 0;
#pragma unroll
    for (int k = 0; k < CC_MAX_MX; ++k) if (k == m) md = p.maxdet[k];
    const unsigned n = ev_live(p.state, p.n_host, p.capacity);
    const unsigned s = ev_class_begin(p.keys, n, c), e = ev_class_begin(p.keys, n, c + 1);
    const int ng = p.npig[(long long)c * p.A + a];
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    auto entry = [&](unsigned i) -> unsigned {       // i < e
        const unsigned w = p.words[(long long)i * p.A + a];
        const bool counts = p.ranks[i] < md && !(w & ig_bit);
        return counts ? ((w & tp_bit) ? 3u : 1u) : 0u;
    };
    unsigned tot_tp = 0;
    q[tid] = 0.0;
    kr[tid] = CC_NO_K;
    if (ng > 0) {                                                         // the same for the whole workgroup
        if (tid < p.R) {                                                  // k_r = the smallest k >= 0 with k / ng >= rec_thr[r]
            const double thr = p.rec_thr[tid], dng = (double)ng;
            int k = CC_NO_K;                                              // a NaN threshold, or a count beyond 2^30: never reached
            if (thr <= 0.0) k = 0;
            else if (thr * dng < 1073741824.0) {
                // the exact answer is ceil(thr ng) or one less (the division may round up to thr); floor(fl(thr ng)) - 1 is
                // at most that and at least two below it.  (Nothing bounds k by ng: the entries decide whether a count occurs.)
                long long k0 = (long long)floor(thr * dng) - 1;
                k0 = k0 < 0 ? 0 : k0;
                for (int dk = 3; dk >= 0; --dk) {
                    const long long kk = k0 + dk;
                    if ((double)kk / dng >= thr) k = (int)kk;
                }
            }
            kr[tid] = k;
        }
        unsigned rem_n = 0, rem_tp = 0;                                   // entries that count / true positives, whole segment
        for (unsigned i0 = s; i0 < e; i0 += CC_THREADS * 256) {          // a thread adds up to 256 entries before the sums are unpacked
            unsigned tot = 0;
            unsigned i = i0 + tid;
            for (unsigned r = 0; r < 256 && i < e; ++r, i += CC_THREADS) {
                const unsigned f = entry(i);
                tot += (f & 1u) + ((f & 2u) ? 0x10000u : 0u);
            }
            rem_n += ev_block_sum<unsigned>(tot & 0xFFFFu, shu, tid);
            rem_tp += ev_block_sum<unsigned>(tot >> 16, shu, tid);
        }
        tot_tp = rem_tp;
        __syncthreads();                                                  // kr and q are written
        double carry = 0.0;                                               // largest precision of the chunks behind this one
        const unsigned nchunks = (e - s + EV_AP_CHUNK - 1) / EV_AP_CHUNK;
        for (unsigned ch = nchunks; ch-- > 0;) {
            const unsigned i0 = s + ch * EV_AP_CHUNK + (unsigned)tid * EV_AP_ITEMS;
            unsigned f[EV_AP_ITEMS], cnt = 0;
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r) {
                f[r] = i0 + r < e ? entry(i0 + r) : 0u;
                cnt += (f[r] & 1u) + ((f[r] & 2u) ? 0x10000u : 0u);
            }
            unsigned total;
            const unsigned ex = fo_block_excl_scan(cnt, shu, tid, &total);
            rem_n -= total & 0xFFFFu; rem_tp -= total >> 16;              // now: the counts in front of this chunk
            unsigned rank = rem_n + (ex & 0xFFFFu), ctp = rem_tp + (ex >> 16);
            double prec[EV_AP_ITEMS];
            unsigned at_rank[EV_AP_ITEMS], at_tp[EV_AP_ITEMS];
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r) {
                rank += f[r] & 1u; ctp += (f[r] >> 1) & 1u;
                at_rank[r] = rank; at_tp[r] = ctp;
                prec[r] = (f[r] & 1u) ? (double)ctp / ((double)rank + 0x1p-52) : 0.0;      // (fp + tp) + eps: rank is their exact sum
            }
#pragma unroll
            for (int r = EV_AP_ITEMS - 2; r >= 0; --r) prec[r] = fmax(prec[r], prec[r + 1]);      // envelope inside the thread
            double chunk_max;
            const double later = fmax(ev_block_excl_rmax(prec[0], shd, tid, &chunk_max), carry);
#pragma unroll
            for (int r = 0; r < EV_AP_ITEMS; ++r) {
                if (!(f[r] & 1u)) continue;
                const double env = fmax(prec[r], later);
                if (at_rank[r] == 1u)                                     // the first entry: every threshold that the count 0 reaches
                    for (int x = 0; x < p.R && kr[x] == 0; ++x) q[x] = env;
                if (f[r] & 2u) {
                    const int k = (int)at_tp[r];
                    for (int x = (int)fo_partition_point(kr, (unsigned)p.R, [=](int v) { return v < k; }); x < p.R && kr[x] == k; ++x)
                        q[x] = env;
                }
            }
            carry = fmax(carry, chunk_max);
        }
    }
    __syncthreads();                                                      // q is complete
    const long long cell = (((long long)t * p.C + c) * p.A + a) * p.Mx + m, cells = (long long)p.T * p.C * p.A * p.Mx;
    if (p.precision && tid < p.R)
        p.precision[((((long long)t * p.R + tid) * p.C + c) * p.A + a) * p.Mx + m] = ng > 0 ? q[tid] : __builtin_nan("");
    if (tid != 0) return;
    double* ap = reinterpret_cast<double*>(p.result + CC_RESULT_HEAD);
    double sum = 0.0;
    for (int r = 0; r < p.R; ++r) sum = sum + q[r];                       // ascending r, one addition each
    ap[cell] = ng > 0 ? sum / (double)p.R : __builtin_nan("");
    ap[cells + cell] = ng > 0 ? (double)tot_tp / (double)ng : __builtin_nan("");
    if (t == 0 && m == 0) reinterpret_cast<long long*>(p.result)[CC_RESULT_HEAD + 2 * cells + (long long)c * p.A + a] = ng;
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        p.result[0] = n; p.result[1] = p.state ? p.state[1] : 0; p.result[2] = p.state ? p.state[2] : 0;
        p.result[3] = (u64)p.T; p.result[4] = (u64)p.C; p.result[5] = (u64)p.A; p.result[6] = (u64)p.Mx; p.result[7] = (u64)p.R;
    }
}

// ---- workspace layout (host) -------------------------------------------------------------------------------------------------------
// the sort's buffers, then the gathered words [capacity][A] and ranks [capacity]
bool cc_layout(long long capacity, int C, int A, EvLayout* L) { return A >= 1 && A <= EM_MAX_A && ev_layout(capacity, C, 4ll * A, 4, L); }

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int effdet_coco_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                                 const unsigned char* gt_crowd, const float* gt_area, int B, int max_det, int M, int num_classes,
                                 const float* thresholds, int num_thresholds, const float* area_ranges, int num_areas,
                                 int max_rank, float min_score, unsigned int* flags, int* rank, int* kept, int* npig) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !area_ranges || !flags || !rank || !npig)
        return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, EM_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15, ascending, no NaN
    if (!em_areas_ok(area_ranges, num_areas)) return EFFDET_EINVAL;      // 1 <= num_areas <= 4, an area range needs lo <= hi
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    if (max_rank < 1) return EFFDET_EINVAL;      // max_rank (the largest max_dets) must be positive
    if (min_score != min_score) return EFFDET_EINVAL;      // min_score is NaN
    const size_t sh = cc_match_lds(M, num_classes);
    if (sh > 64 * 1024) return EFFDET_EINVAL;      // 40 M + 4 num_classes bytes exceed 64 KiB of LDS
    CcMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_crowd = gt_crowd; a.gt_area = gt_area;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds; a.A = num_areas; a.max_rank = max_rank;
    a.min_score = min_score;
    for (int t = 0; t < EM_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    for (int k = 0; k < EM_MAX_A; ++k) { a.lo[k] = k < num_areas ? area_ranges[2 * k] : 0.f; a.hi[k] = k < num_areas ? area_ranges[2 * k + 1] : 0.f; }
    a.flags = flags; a.rank = rank; a.kept = kept; a.npig = npig;
    hipLaunchKernelGGL(cc_match_kernel, dim3(B), dim3(CC_THREADS), sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_coco_append(void* stream, const float* det, const unsigned int* flags, const int* rank, const int* kept, int B,
                                  int max_det, int num_areas, float* scores, int* classes, unsigned int* words, int* ranks,
                                  long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !rank || !kept || !scores || !classes || !words || !ranks || !state) return EFFDET_EINVAL;      // null pointer
    if (!em_slots_ok(B, max_det)) return EFFDET_EINVAL;      // bad B or max_det
    if (num_areas < 1 || num_areas > EM_MAX_A) return EFFDET_EINVAL;      // 1 <= num_areas <= 4
    if (!ev_capacity_ok(capacity)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    const CcAppend a{{det, kept, B, max_det, scores, classes, (unsigned)capacity, state}, flags, rank, num_areas, words, ranks};
    return ev_append(stream, a);
}

extern "C" long long effdet_coco_sorted_workspace_bytes(long long capacity, int num_classes, int num_areas) {
    EvLayout L;
    return cc_layout(capacity, num_classes, num_areas, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_coco_sorted_offset(long long capacity, int num_classes, int num_areas, int which) {
    EvLayout L;
    if (which < 0 || which > 3 || !cc_layout(capacity, num_classes, num_areas, &L)) return EFFDET_EINVAL;
    return which == 0 ? L.keys[ev_last(L)] : which == 1 ? L.vals[ev_last(L)] : L.extra[which - 2];
}

extern "C" long long effdet_coco_sorted_result_bytes(int num_thresholds, int num_classes, int num_areas, int num_max_dets) {
    if (num_thresholds < 1 || num_thresholds > EM_MAX_T || !em_classes_ok(num_classes) || num_areas < 1 || num_areas > EM_MAX_A ||
        num_max_dets < 1 || num_max_dets > CC_MAX_MX)
        return EFFDET_EINVAL;
    return 8ll * (CC_RESULT_HEAD + 2ll * num_thresholds * num_classes * num_areas * num_max_dets + (long long)num_classes * num_areas);
}

extern "C" int effdet_coco_sorted(void* stream, const float* scores, const int* classes, const unsigned int* words, const int* ranks,
                                  long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes,
                                  int num_areas, const int* max_dets, int num_max_dets, const double* rec_thr, int num_rec,
                                  const int* npig, void* workspace, long long workspace_bytes, void* result, double* precision) {
    EFFDET_ENTER();
    if (!scores || !classes || !words || !ranks || !max_dets || !rec_thr || !npig || !workspace || !result)
        return EFFDET_EINVAL;      // null pointer
    if (n < 0 && !state) return EFFDET_EINVAL;      // n < 0 takes the count from `state`, which is null
    if (num_thresholds < 1 || num_thresholds > EM_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15
    if (num_max_dets < 1 || num_max_dets > CC_MAX_MX) return EFFDET_EINVAL;      // 1 <= num_max_dets <= 4
    for (int k = 0; k < num_max_dets; ++k)
        if (max_dets[k] < 1 || (k > 0 && max_dets[k] <= max_dets[k - 1])) return EFFDET_EINVAL;      // max_dets must be positive and ascend
    if (num_rec < 1 || num_rec > CC_MAX_R) return EFFDET_EINVAL;      // 1 <= num_rec <= 256
    EvLayout L;
    if (!cc_layout(capacity, num_classes, num_areas, &L)) return EFFDET_EINVAL;      // capacity in [1, 2^24], classes in [1, 65535], areas in [1, 4]
    if (n > capacity) return EFFDET_EINVAL;      // n exceeds the capacity
    if (workspace_bytes < L.total) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(result) % 8 || reinterpret_cast<uintptr_t>(rec_thr) % 8 ||
        reinterpret_cast<uintptr_t>(precision) % 8)
        return EFFDET_EINVAL;      // workspace, result, rec_thr and precision must be 8-byte aligned
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long n_host = n < 0 ? -1 : n;
    const unsigned grid = ev_sort(st, CcSort(), scores, classes, state, n_host, capacity, num_classes, ws, L, [](CcSort&, int) {});
    const int last = ev_last(L);
    CcGather g;
    g.index = reinterpret_cast<const unsigned*>(ws + L.vals[last]); g.words = words; g.ranks = ranks;
    g.cursor = state; g.n_host = n_host; g.capacity = (unsigned)capacity; g.A = num_areas;
    g.out_words = reinterpret_cast<unsigned*>(ws + L.extra[0]); g.out_ranks = reinterpret_cast<int*>(ws + L.extra[1]);
    if (grid > 0) hipLaunchKernelGGL(cc_gather_kernel, dim3(grid * (RS_TILE / CC_THREADS)), dim3(CC_THREADS), 0, st, g);
    CcAp a;
    a.keys = reinterpret_cast<const u64*>(ws + L.keys[last]); a.words = g.out_words; a.ranks = g.out_ranks;
    a.state = state; a.n_host = n_host; a.capacity = (unsigned)capacity;
    a.T = num_thresholds; a.C = num_classes; a.A = num_areas; a.Mx = num_max_dets; a.R = num_rec;
    for (int k = 0; k < CC_MAX_MX; ++k) a.maxdet[k] = k < num_max_dets ? max_dets[k] : 0;
    a.rec_thr = rec_thr; a.npig = npig; a.result = reinterpret_cast<u64*>(result); a.precision = precision;
    hipLaunchKernelGGL(cc_ap_kernel, dim3((unsigned)num_classes, (unsigned)(num_thresholds * num_areas * num_max_dets)), dim3(CC_THREADS),
                       0, st, a);
    return effdet_check_launch();
}
