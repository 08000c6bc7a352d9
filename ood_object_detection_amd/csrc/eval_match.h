// What the greedy matchers state once.  One workgroup of EM_THREADS threads per image.
//   evaluation.hip (one threshold, a `tp` label per slot), eval_scale.hip (up to 16 thresholds, a flag word per slot, and its open
//   words): the float32 IoU, the staging of an image's ground truth with its per-class counters (em_stage_gt) and the search for
//   a detection's candidate box (em_best_box).  What thread 0 does with the candidate differs between the kernels and stays there.
//   coco_eval.hip, lvis_eval.hip (the COCO rule per (IoU threshold, area range) pair, A flag words per slot): the IoU, the limits
//   and the flag bits, and the walk of a detection's IoU row by the lane that owns a pair (em_walk_row).  The staging, the row and
//   the verdict are written out in both kernels: stated once here they compiled to slower kernels (profiles/README.md, eval_shared_*).
//   All four units: the host-side argument checks of their C ABI (em_slots_ok, em_classes_ok, em_thresholds_ok, em_areas_ok).
//
// The units are compiled with -ffp-contract=off: the IoU must round like the reference's separate float32 numpy operations
// (effdet/evaluation/np_box_ops.py), so its operations stay in this order, one rounding each.
#pragma once
#include "common.h"

namespace {

constexpr int EM_THREADS = 256;
constexpr int EM_NO_BOX = 0x7fffffff;                           // the candidate index of a detection whose class has no box

struct EmDet { float x1, y1, x2, y2, area; };
DEV EmDet em_det(float x1, float y1, float x2, float y2) { return EmDet{x1, y1, x2, y2, (y2 - y1) * (x2 - x1)}; }

// IoU of a detection and the ground-truth box (g0, g1, g2, g3) = (ymin, xmin, ymax, xmax)
DEV float em_iou(const EmDet& d, float g0, float g1, float g2, float g3) {
    const float ih = fmaxf(0.f, fminf(d.y2, g2) - fmaxf(d.y1, g0));
    const float iw = fmaxf(0.f, fminf(d.x2, g3) - fmaxf(d.x1, g1));
    const float inter = ih * iw;
    const float area_g = (g2 - g0) * (g3 - g1);
    return inter / (d.area + area_g - inter);
}
// against a COCO crowd region (coco_eval.hip): the same intersection over the detection's own area
DEV float em_iou_crowd(const EmDet& d, float g0, float g1, float g2, float g3) {
    const float ih = fmaxf(0.f, fminf(d.y2, g2) - fmaxf(d.y1, g0));
    const float iw = fmaxf(0.f, fminf(d.x2, g3) - fmaxf(d.x1, g1));
    return (ih * iw) / d.area;
}

// ---- the COCO rule (coco_eval.hip:6-25), for coco_eval.hip and lvis_eval.hip ------------------------------------------------------
constexpr int EM_MAX_T = 15, EM_MAX_A = 4;                      // T A <= 60 pairs: a lane of wave 0 each, a bit of `taken` each
constexpr unsigned EM_DROPPED = 0x80000000u;                    // a slot's flag words: bit t true positive, bit 16 + t ignored, bit 31
constexpr int EM_ROW_CROWD = 1 << 4, EM_ROW_OF_CLASS = 1 << 5;  // box bits beside the ignore bits 0 .. A-1

// The lane that owns pair (t, a) of coco_eval.hip / lvis_eval.hip walks the detection's IoU row in LDS.  rmeta[j]: 0 for a box of
// another class, else EM_ROW_OF_CLASS | EM_ROW_CROWD (a crowd region) | bit a (ignored at area range a); taken[j] bit `pair`: taken
// at this pair (a crowd region stays free).  -> *free_box: the box not ignored at a with the largest IoU >= thr, the LAST index on
// equal IoU (>=); *ign_box: the same among the ignored boxes; -1 where there is none.  Every lane reads the same words: broadcasts.
DEV void em_walk_row(const int* rmeta, const unsigned long long* taken, const float* iou, int M, int pair, int a, float thr,
                     int* free_box, int* ign_box) {
    int b1 = -1, b2 = -1;
    float v1 = thr, v2 = thr;
    for (int j = 0; j < M; ++j) {
        const int m = rmeta[j];
        if (!(m & EM_ROW_OF_CLASS)) continue;
        if (!(m & EM_ROW_CROWD) && ((taken[j] >> pair) & 1ull)) continue;
        const float v = iou[j];
        if ((m >> a) & 1) { if (v >= v2) { v2 = v; b2 = j; } }
        else { if (v >= v1) { v1 = v; b1 = j; } }
    }
    *free_box = b1; *ign_box = b2;
}


// ---- the PASCAL matchers (evaluation.hip, eval_scale.hip) -----------------------------------------------------------------------------
// All threads call it, once, before the first search.  LDS: seen[C] = 0 (class already had its top-scoring detection), taken[M] = 0,
// gcls[M] = the 0-based class of box j of image b or -1, and, when gdif is given, gdif[M] = the box is `difficult` (gt_difficult
// may be null: none is).  Then the counters, by integer atomics (order independent): gt_count[c] += boxes of class c - with gdif,
// those that are not difficult (object_detection_evaluation.py:132-139) - and gt_imgs[c] += 1 when class c occurs in the image at all.
DEV void em_stage_gt(const long long* gt_cls, const unsigned char* gt_difficult, int b, int M, int C, int* seen, int* taken, int* gcls,
                     int* gdif, int* gt_count, int* gt_imgs) {
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += EM_THREADS) seen[c] = 0;
    for (int j = tid; j < M; j += EM_THREADS) {
        const long long c1 = gt_cls[(long long)b * M + j];
        gcls[j] = (c1 >= 1 && c1 <= C) ? (int)(c1 - 1) : -1;
        if (gdif) gdif[j] = (gt_difficult && gt_difficult[(long long)b * M + j]) ? 1 : 0;
        taken[j] = 0;
    }
    __syncthreads();
    for (int j = tid; j < M; j += EM_THREADS) {
        const int c = gcls[j];
        if (c < 0) continue;
        if (!gdif || !gdif[j]) atomicAdd(gt_count + c, 1);
        bool first = true;
        for (int q = 0; q < j; ++q) first = first && gcls[q] != c;
        if (first) atomicAdd(gt_imgs + c, 1);
    }
}

// All threads call it, with the same detection.  Among the boxes of image b whose class is c: the one with the largest IoU, the
// lowest index on ties.  The result is valid on thread 0 only: the index (EM_NO_BOX: no box of class c) and *iou (-1 then).
// red_v, red_i: [EM_THREADS / 64] in LDS.  It contains barriers; the caller's barrier at the end of its round frees red_v / red_i.
DEV int em_best_box(const EmDet& d, int c, const float* gt_boxes, const int* gcls, int b, int M, float* red_v, int* red_i, float* iou) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float best = -1.f; int bj = EM_NO_BOX;
    for (int j = tid; j < M; j += EM_THREADS) {
        if (gcls[j] != c) continue;
        const float* g = gt_boxes + ((long long)b * M + j) * 4;                 // yxyx
        const float v = em_iou(d, g[0], g[1], g[2], g[3]);
        if (v > best) { best = v; bj = j; }                                     // ascending j: first maximum kept
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov > best || (ov == best && oj < bj)) { best = ov; bj = oj; }
    }
    __syncthreads();
    if (lane == 0) { red_v[wave] = best; red_i[wave] = bj; }
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < EM_THREADS / 64; ++w)
            if (red_v[w] > best || (red_v[w] == best && red_i[w] < bj)) { best = red_v[w]; bj = red_i[w]; }
    *iou = best;
    return bj;
}

// ---- host: the argument checks of the units' C ABI -----------------------------------------------------------------------------------
constexpr long long EM_MAX_N = 1ll << 24;                       // slots of a call, entries of a buffer
constexpr int EM_MAX_C = 65535;
// B images of max_det slots
bool em_slots_ok(int B, int max_det) { return B > 0 && max_det > 0 && (long long)B * max_det <= EM_MAX_N; }
bool em_classes_ok(int num_classes, int least = 1) { return num_classes >= least && num_classes <= EM_MAX_C; }
// 1 .. max_T thresholds, none NaN, ascending
bool em_thresholds_ok(const float* thr, int T, int max_T) {
    if (T < 1 || T > max_T) return false;
    for (int t = 0; t < T; ++t)
        if (!(thr[t] == thr[t]) || (t > 0 && !(thr[t] > thr[t - 1]))) return false;
    return true;
}
// 1 .. EM_MAX_A area ranges [A][2], lo <= hi each (a NaN bound is refused)
bool em_areas_ok(const float* area_ranges, int A) {
    if (A < 1 || A > EM_MAX_A) return false;
    for (int a = 0; a < A; ++a)
        if (!(area_ranges[2 * a] <= area_ranges[2 * a + 1])) return false;
    return true;
}

}  // namespace
