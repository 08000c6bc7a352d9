// LVIS federated detection evaluation on the device: LVISEval.evaluate_img for a whole batch in one launch.  The
// accumulate stage is coco_eval.hip's: the four outputs below have the layout of effdet_coco_match, so effdet_coco_append and
// effdet_coco_sorted take them unchanged.  Compiled with -ffp-contract=off: the IoU rounds like eval_match.h's separate float32
// operations.
//
// Definitions (restated in tests/_lvis_eval_ref.py; what is not said here is as in coco_eval.hip:6-25).  Per image b: det
// [max_det][6] rows x1, y1, x2, y2, score, 1-based class IN ANY ORDER, count[b] valid rows; ground truth boxes yxyx with a 1-based
// class (<= 0: padding) and an area (null: the float32 box area); neg_cls [Kn] and nel_cls [Ke], int64 1-based category lists
// (<= 0: padding): the categories checked absent in the image and the categories not exhaustively annotated in it.  A null neg_cls:
// every category is judged in every image; a null nel_cls: no category is not-exhaustive.  pos(b): the classes of the image's own
// boxes.  There are no crowd boxes.
//   valid     slot i is valid iff i < count, the box is not degenerate (y1 < y2 && x1 < x2), the class lies in 1..C, the score is
//             not NaN and not < min_score.
//   rank      r_i = the number of valid slots j of the image with score_j > score_i, or score_j == score_i and j < i.  Slot i is
//             dropped iff r_i >= max_rank (max_dets[-1]: LVIS's cap of 300 detections an image over ALL categories).  The cap
//             comes before the filter: a detection of a category that is not judged still uses up a place.  The stored rank is
//             r_i, so `rank < max_dets[m]` nests for several max_dets.
//   filter    a slot that survived the cap is dropped iff its class is in neither pos(b) nor neg(b).
//   matching  per (t, a) the kept slots in ascending r_i (not in slot order), by coco_eval.hip's greedy rule without a crowd box:
//             the best box not yet taken and not ignored at a, the last index on equal IoU; failing that the best untaken
//             ignored box; a matched box is always taken.
//   unmatched ignored at (t, a) iff the detection's own box area lies outside [lo_a, hi_a] OR its class is in nel(b); otherwise
//             a false positive.  A matched detection of a nel category is a true positive or ignored as the matching decides.
//   output    flags [B][max_det][A] (bit t: true positive, bit 16 + t: ignored, bit 31: dropped), rank [B][max_det] (-1: dropped),
//             kept [2 B] (kept slots of image b, then its NaN scores), npig [C][A] by integer atomics.
//
// Kernel: one workgroup of 256 threads per image.  LDS, 40 M + 12 ceil(C / 32) + 8 max_det + 16 bytes (<= 64 KiB):
//   the image's boxes, classes, ignore bits and `taken` words, as cc_match_kernel stages them (40 M);
//   three bitsets over C: pos (from the staged classes), neg and nel (from the lists), set by integer LDS atomics;
//   score [max_det]: the slot's score, NaN for a slot that is not valid, so that one float comparison per pair ranks;
//   inv [max_det]: rank -> slot for the kept slots, -1 elsewhere, so that the walk runs in rank order.
// Thread i % 256 ranks slot i against the max_det scores in LDS (max_det^2 / 256 comparisons a thread: 352 at 300), writes the
// dropped slots' words at once and enters the kept ones in inv.  Then the workgroup walks r = 0 .. min(max_det, max_rank) - 1: the
// IoU row of slot inv[r] against the boxes of its class goes to LDS, lane (t, a) of wave 0 walks it (em_walk_row), two ballots turn
// the lanes' verdicts into the A flag words.  max_det <= 2048 (LV_MAX_DET): 16 KiB for score and inv, 16 384 comparisons a thread.
// No floating-point atomics; every loop has a trip count known at its entry; every index is compared with its extent before a
// store; no host synchronisation; the launch is capturable; the results do not depend on the order in which threads run.
#include "common.h"
#include "compact.h"
#include "eval_match.h"

namespace {

typedef unsigned long long u64;

constexpr int LV_THREADS = 256;
static_assert(LV_THREADS == FO_THREADS && LV_THREADS == EM_THREADS, "the shared headers are written for this workgroup size");
constexpr int LV_MAX_DET = 2048;

struct LvMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls; const float* gt_area;
    const long long* neg_cls; const long long* nel_cls;
    int B, max_det, M, C, T, A, max_rank, Kn, Ke; float min_score; float thr[EM_MAX_T]; float lo[EM_MAX_A], hi[EM_MAX_A];
    unsigned* flags; int* rank; int* kept; int* npig;
};

long long lv_match_lds(int max_det, int M, int C) {
    if (max_det < 1 || max_det > LV_MAX_DET || M < 1 || !em_classes_ok(C)) return EFFDET_EINVAL;
    return 40ll * M + 12ll * ((C + 31) / 32) + 8ll * max_det + 16;
}

// the 0-based class of a detection row's class column, -1 outside 1..C (NaN included)
DEV int lv_class(float cf, int C) { return (cf >= 1.f && cf < (float)(C + 1)) ? (int)cf - 1 : -1; }

// the members 1..C of list[0 .. K) into the bitset
DEV void lv_fill_set(const long long* list, int K, int C, unsigned* set, int tid) {
    for (int k = tid; k < K; k += LV_THREADS) {
        const long long c1 = list[k];
        if (c1 >= 1 && c1 <= C) atomicOr(&set[(int)(c1 - 1) >> 5], 1u << ((int)(c1 - 1) & 31));
    }
}

__global__ __launch_bounds__(LV_THREADS) void lv_match_kernel(LvMatch p) {
    extern __shared__ double lv_lds[];
    const int W = (p.C + 31) >> 5;
    u64* taken = reinterpret_cast<u64*>(lv_lds);                  // [M] bit t A + a: taken at (t, a)
    float* box = reinterpret_cast<float*>(taken + p.M);           // [M][4] yxyx
    float* iou = box + 4 * p.M;                                   // [M] the detection's row
    int* gcls = reinterpret_cast<int*>(iou + p.M);                // [M] 0-based class or -1
    int* gmeta = gcls + p.M;                                      // [M] bit a: ignored at a
    int* rmeta = gmeta + p.M;                                     // [M] gmeta | EM_ROW_OF_CLASS for the boxes of the detection's class, else 0
    unsigned* pos = reinterpret_cast<unsigned*>(rmeta + p.M);     // [W] classes of the image's boxes
    unsigned* neg = pos + W;                                      // [W] categories checked absent
    unsigned* nel = neg + W;                                      // [W] categories not exhaustively annotated
    float* score = reinterpret_cast<float*>(nel + W);             // [max_det] NaN: the slot is not valid
    int* inv = reinterpret_cast<int*>(score + p.max_det);         // [max_det] rank -> kept slot, -1: none
    unsigned* shu = reinterpret_cast<unsigned*>(inv + p.max_det); // [4] the scan's scratch
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int w = tid; w < 3 * W; w += LV_THREADS) pos[w] = 0u;    // pos, neg and nel are contiguous
    for (int i = tid; i < p.max_det; i += LV_THREADS) inv[i] = -1;
    __syncthreads();
    for (int j = tid; j < p.M; j += LV_THREADS) {
        const long long at = (long long)b * p.M + j;
        const long long c1 = p.gt_cls[at];
        const int cls = (c1 >= 1 && c1 <= p.C) ? (int)(c1 - 1) : -1;
        const float* g = p.gt_boxes + at * 4;
        const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
        box[4 * j] = g0; box[4 * j + 1] = g1; box[4 * j + 2] = g2; box[4 * j + 3] = g3;
        const float area = p.gt_area ? p.gt_area[at] : (g2 - g0) * (g3 - g1);
        int meta = 0;
#pragma unroll
        for (int a = 0; a < EM_MAX_A; ++a) {
            if (a >= p.A) continue;
            const bool ig = area < p.lo[a] || area > p.hi[a];
            meta |= (ig ? 1 : 0) << a;
            if (cls >= 0 && !ig) atomicAdd(p.npig + (long long)cls * p.A + a, 1);
        }
        if (cls >= 0) atomicOr(&pos[cls >> 5], 1u << (cls & 31));
        gcls[j] = cls; gmeta[j] = meta; taken[j] = 0;
    }
    if (p.neg_cls) lv_fill_set(p.neg_cls + (long long)b * p.Kn, p.Kn, p.C, neg, tid);
    if (p.nel_cls) lv_fill_set(p.nel_cls + (long long)b * p.Ke, p.Ke, p.C, nel, tid);
    // validity: score[i] is the slot's score, NaN when the slot is not valid
    const int n = min(p.det_count[b], p.max_det);
    unsigned nans = 0;
    for (int i = tid; i < p.max_det; i += LV_THREADS) {
        const float* d = p.det + ((long long)b * p.max_det + i) * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], s = d[4];
        const bool ok = i < n && y1 < y2 && x1 < x2 && lv_class(d[5], p.C) >= 0 && s == s && !(s < p.min_score);
        if (i < n && s != s) ++nans;
        score[i] = ok ? s : __builtin_nanf("");
    }
    __syncthreads();                                              // the sets, the staged boxes and the scores are complete
    // image rank, cap, federated filter
    unsigned kept = 0;
    for (int i = tid; i < p.max_det; i += LV_THREADS) {
        const long long slot = (long long)b * p.max_det + i;
        const float s = score[i];
        int r = -1;
        bool keep = false;
        if (s == s) {
            r = 0;
            for (int j = 0; j < p.max_det; ++j) {                // a NaN never counts
                const float v = score[j];
                r += (v > s || (v == s && j < i)) ? 1 : 0;
            }
            const int c = lv_class(p.det[slot * 6 + 5], p.C);     // >= 0: the slot is valid
            const unsigned bit = 1u << (c & 31);
            keep = r < p.max_rank && r < p.max_det && c >= 0 && (!p.neg_cls || ((pos[c >> 5] | neg[c >> 5]) & bit));
        }
        if (keep) {
            inv[r] = i;                                           // ranks of valid slots are distinct: one writer
            p.rank[slot] = r;
            ++kept;
        } else {
            for (int a = 0; a < p.A; ++a) p.flags[slot * p.A + a] = EM_DROPPED;
            p.rank[slot] = -1;
        }
    }
    unsigned tot_kept, tot_nans;
    fo_block_excl_scan(kept, shu, tid, &tot_kept);                // its barriers also publish inv
    fo_block_excl_scan(nans, shu, tid, &tot_nans);
    if (tid == 0 && p.kept) { p.kept[b] = (int)tot_kept; p.kept[p.B + b] = (int)tot_nans; }
    // lane `pair` of wave 0 owns (t, a)
    const int pair = tid & 63;
    const bool active = tid < 64 && pair < p.T * p.A;
    const int my_t = pair / p.A, my_a = pair % p.A;
    float my_thr = 0.f, my_lo = 0.f, my_hi = 0.f;
#pragma unroll
    for (int t = 0; t < EM_MAX_T; ++t) if (t == my_t) my_thr = p.thr[t];
#pragma unroll
    for (int a = 0; a < EM_MAX_A; ++a) if (a == my_a) { my_lo = p.lo[a]; my_hi = p.hi[a]; }
    const int walk = min(p.max_det, p.max_rank);
    for (int r = 0; r < walk; ++r) {
        const int i = inv[r];
        if (i < 0 || i >= p.max_det) continue;                    // a rank whose slot the filter dropped, or none: the same for the whole workgroup
        const long long slot = (long long)b * p.max_det + i;
        const float* d = p.det + slot * 6;
        const int c = lv_class(d[5], p.C);
        if (c < 0) continue;                                      // never: a kept slot is valid
        const bool not_exh = (nel[c >> 5] >> (c & 31)) & 1u;
        const EmDet dd = em_det(d[0], d[1], d[2], d[3]);
        for (int j = tid; j < p.M; j += LV_THREADS) {
            int m = 0;
            if (gcls[j] == c) {
                m = gmeta[j] | EM_ROW_OF_CLASS;
                const float* g = box + 4 * j;
                iou[j] = em_iou(dd, g[0], g[1], g[2], g[3]);
            }
            rmeta[j] = m;
        }
        __syncthreads();
        if (tid < 64) {
            int b1 = -1, b2 = -1;                                 // the best box not ignored / ignored at my_a
            if (active) em_walk_row(rmeta, taken, iou, p.M, pair, my_a, my_thr, &b1, &b2);
            const int bj = b1 >= 0 ? b1 : b2;
            const bool tp = active && b1 >= 0;
            const bool ign = active && b1 < 0 && (b2 >= 0 || dd.area < my_lo || dd.area > my_hi || not_exh);
            if (active && bj >= 0) atomicOr(&taken[bj], (u64)(1ull << pair));
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
        }
        __syncthreads();                                          // the row and `taken` are settled for the next detection
    }
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_lvis_match_lds_bytes(int max_det, int M, int num_classes) { return lv_match_lds(max_det, M, num_classes); }

extern "C" int effdet_lvis_match(void* stream, const float* det, const int* det_count, const float* gt_boxes, const long long* gt_cls,
                                 const float* gt_area, int B, int max_det, int M, int num_classes, const float* thresholds,
                                 int num_thresholds, const float* area_ranges, int num_areas, int max_rank, float min_score,
                                 const long long* neg_cls, int Kn, const long long* nel_cls, int Ke, unsigned int* flags, int* rank,
                                 int* kept, int* npig) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !area_ranges || !flags || !rank || !npig)
        return EFFDET_EINVAL;      // null pointer
    if (!em_thresholds_ok(thresholds, num_thresholds, EM_MAX_T)) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 15, ascending, no NaN
    if (!em_areas_ok(area_ranges, num_areas)) return EFFDET_EINVAL;      // 1 <= num_areas <= 4, an area range needs lo <= hi
    if (!em_slots_ok(B, max_det) || M <= 0) return EFFDET_EINVAL;      // bad B, max_det or M
    if (max_det > LV_MAX_DET) return EFFDET_EINVAL;      // max_det exceeds 2048
    if (!em_classes_ok(num_classes)) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    if (max_rank < 1) return EFFDET_EINVAL;      // max_rank (the largest max_dets) must be positive
    if (min_score != min_score) return EFFDET_EINVAL;      // min_score is NaN
    if ((neg_cls && Kn < 0) || (nel_cls && Ke < 0)) return EFFDET_EINVAL;      // a category list of negative length
    const long long sh = lv_match_lds(max_det, M, num_classes);
    if (sh < 0 || sh > 64 * 1024) return EFFDET_EINVAL;      // 40 M + 12 ceil(num_classes / 32) + 8 max_det + 16 bytes exceed 64 KiB of LDS
    LvMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_area = gt_area;
    a.neg_cls = neg_cls; a.nel_cls = nel_cls; a.Kn = neg_cls ? Kn : 0; a.Ke = nel_cls ? Ke : 0;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds; a.A = num_areas; a.max_rank = max_rank;
    a.min_score = min_score;
    for (int t = 0; t < EM_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    for (int k = 0; k < EM_MAX_A; ++k) { a.lo[k] = k < num_areas ? area_ranges[2 * k] : 0.f; a.hi[k] = k < num_areas ? area_ranges[2 * k + 1] : 0.f; }
    a.flags = flags; a.rank = rank; a.kept = kept; a.npig = npig;
    hipLaunchKernelGGL(lv_match_kernel, dim3(B), dim3(LV_THREADS), (size_t)sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}
