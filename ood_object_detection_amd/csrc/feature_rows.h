// What the OOD units that read rows of a [B, K] call share (feature_ood.hip, feature_knn.hip, feature_subspace.hip, logit_ood.hip, act_shaping.hip;
// DESIGN.md §8): which entries count (FoSel), the class label of an entry (FoClasses), the feature rows - F-vectors of pyramid cells
// read through a level table (<= 8 entries: base, cells, batch stride, cell stride; channel stride 1), float32 or bfloat16 -, the
// geometry and staging of the kernels that keep 16 centred rows per wave in LDS, the dispatch on the width, and the host checks of
// these arguments.  The reductions and the ordered compaction are compact.h's.
#pragma once
#include <type_traits>
#include "common.h"
#include "compact.h"

namespace {

constexpr long long FO_MAX_ROWS = 1ll << 27;                    // B * K of one call
constexpr int FO_MAX_LEVELS = 8;

struct FoLevels {
    const void* base[FO_MAX_LEVELS];
    long long bstride[FO_MAX_LEVELS], cstride[FO_MAX_LEVELS];   // elements
    unsigned start[FO_MAX_LEVELS + 1];                          // first cell of level l; start[n] = P
    int n, bf16;
    unsigned P;
};

// first element of the feature row of cell `cell` (< P) of image b
DEV const char* fo_row(const FoLevels& L, unsigned b, unsigned cell) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < FO_MAX_LEVELS; ++k) l += (k < L.n && cell >= L.start[k]) ? 1 : 0;
    const long long off = (long long)b * L.bstride[l] + (long long)(cell - L.start[l]) * L.cstride[l];
    return reinterpret_cast<const char*>(L.base[l]) + off * (L.bf16 ? 2 : 4);
}
// element k of a row; bfloat16 is widened exactly
DEV float fo_ld(const char* row, int k, int bf16) {
    if (bf16) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(row)[k] << 16);
    return reinterpret_cast<const float*>(row)[k];
}

// Which entries of a [B, K] call count: entry i = b * K + j does when j < count[b] (null: all) and its anchor - anchor[i], or j
// without an index - lies in [0, limit): limit = A * P for feature rows (the anchor sits on cell anchor / A), N for logits.
struct FoSel {
    unsigned K, total;                                          // total = B * K
    const long long* anchor;                                    // [B, K] or null (row j is anchor j)
    const void* count; int count64;
    long long limit;
};
// does entry i count?  *b: its image, *an: its anchor; every index is compared before a pointer is formed
DEV bool fo_select(const FoSel& s, unsigned i, unsigned* b, long long* an) {
    if (i >= s.total) return false;
    const unsigned bb = i / s.K, j = i - bb * s.K;
    if (s.count) {
        const long long c = s.count64 ? reinterpret_cast<const long long*>(s.count)[bb] : (long long)reinterpret_cast<const int*>(s.count)[bb];
        if ((long long)j >= c) return false;
    }
    const long long a = s.anchor ? s.anchor[i] : (long long)j;
    if (a < 0 || a >= s.limit) return false;
    *b = bb; *an = a;
    return true;
}
// the feature row of entry i with A anchors a cell, or null when the entry does not count
DEV const char* fo_sel_row(const FoLevels& L, const FoSel& s, int A, unsigned i) {
    unsigned b; long long an;
    if (!fo_select(s, i, &b, &an)) return nullptr;
    return fo_row(L, b, (unsigned)(an / A));
}

// class labels [B, K] (int32, int64 or float32: dtype 0, 1, 2; strided)
struct FoClasses { const void* ptr; int dtype; long long pitch, stride, offset; int C; };
// the label of entry (b, j) less the offset, or -1 when that lies outside [0, C) (ignore labels, NaN, infinities)
DEV int fo_class(const FoClasses& c, unsigned b, unsigned j) {
    const long long at = (long long)b * c.pitch + (long long)j * c.stride;
    long long cl;
    if (c.dtype == 0) cl = reinterpret_cast<const int*>(c.ptr)[at];
    else if (c.dtype == 1) cl = reinterpret_cast<const long long*>(c.ptr)[at];
    else {
        const float v = reinterpret_cast<const float*>(c.ptr)[at];
        if (!(v >= -2147483648.f && v < 2147483648.f)) return -1;           // NaN, infinities
        cl = (long long)v;
    }
    return (cl < c.offset || cl - c.offset >= c.C) ? -1 : (int)(cl - c.offset);
}

// 64 (48 at F = 288) rows per workgroup, 16 per wave, each wave's rows in its own LDS at pitch FP + 4
template <int NT> struct FoRowGeom {
    static constexpr int FP = 16 * NT, PITCH = FP + 4;
    static constexpr int WAVES = 64 * PITCH * 4 <= 65536 ? 4 : 3;         // LDS of a workgroup stays within 64 KB at every width
    static constexpr int ROWS = 16 * WAVES;
};
// xc = f - mu0 of the wave's 16 entries row0 .. row0 + 15 -> xs (its own LDS rows; zero beyond F and in rows that do not count);
// bit rr of the result: entry row0 + rr counts
template <int NT> DEV unsigned fo_stage_centered(const FoLevels& L, const FoSel& s, int A, int F, const float* mu0, unsigned row0,
                                                 float* xs, int lane) {
    constexpr int FP = FoRowGeom<NT>::FP, PITCH = FoRowGeom<NT>::PITCH;
    unsigned valid = 0;
    for (int rr = 0; rr < 16; ++rr) {
        const char* p = fo_sel_row(L, s, A, row0 + rr);         // the same for the whole wave
        if (p) valid |= 1u << rr;
        for (int k = lane; k < FP; k += 64) xs[rr * PITCH + k] = (p && k < F) ? fo_ld(p, k, L.bf16) - mu0[k] : 0.f;
    }
    return valid;
}

// ---- host ----
bool fo_width_ok(int F) { return F == 64 || F == 88 || F == 112 || F == 160 || F == 224 || F == 288; }

// fn(std::integral_constant<int, NT>{}) for the NT = F / 16 (rounded up) of a supported width
template <typename Fn> void fo_for_width(int F, Fn fn) {
    switch ((F + 15) / 16) {
        case 4: fn(std::integral_constant<int, 4>{}); break;
        case 6: fn(std::integral_constant<int, 6>{}); break;
        case 7: fn(std::integral_constant<int, 7>{}); break;
        case 10: fn(std::integral_constant<int, 10>{}); break;
        case 14: fn(std::integral_constant<int, 14>{}); break;
        default: fn(std::integral_constant<int, 18>{}); break;
    }
}

// the table of the ABI -> the kernels' copy; false: a bad table
bool fo_levels(int dtype, int num_levels, const void* const* bases, const long long* cells, const long long* batch_strides,
               const long long* cell_strides, const long long* channel_strides, int B, FoLevels* L) {
    if ((dtype != EFFDET_F32 && dtype != EFFDET_BF16) || num_levels < 1 || num_levels > FO_MAX_LEVELS) return false;
    if (!bases || !cells || !batch_strides || !cell_strides || !channel_strides || B < 1) return false;
    long long P = 0;
    for (int l = 0; l < FO_MAX_LEVELS; ++l) { L->base[l] = nullptr; L->bstride[l] = 0; L->cstride[l] = 0; L->start[l] = 0; }
    for (int l = 0; l < num_levels; ++l) {
        if (!bases[l] || cells[l] < 1 || batch_strides[l] < 0 || cell_strides[l] < 0 || channel_strides[l] != 1) return false;
        L->base[l] = bases[l]; L->bstride[l] = batch_strides[l]; L->cstride[l] = cell_strides[l];
        L->start[l] = (unsigned)P;
        P += cells[l];
        if (P * B > (1ll << 31)) return false;
    }
    for (int l = num_levels; l <= FO_MAX_LEVELS; ++l) L->start[l] = (unsigned)P;
    L->n = num_levels; L->bf16 = dtype == EFFDET_BF16; L->P = (unsigned)P;
    return true;
}

// the [B, K] arguments of the ABI -> the kernels' copy; false: refuse (limit < 1 covers A < 1 and N < 1)
bool fo_sel(int B, long long K, const long long* anchor_index, const void* count, int count_is_int64, long long limit, FoSel* s) {
    if (B < 1 || K < 1 || (long long)B * K > FO_MAX_ROWS || limit < 1) return false;
    *s = FoSel{(unsigned)K, (unsigned)((long long)B * K), anchor_index, count, count_is_int64 ? 1 : 0, limit};
    return true;
}
// the width, the level table and the rows of a feature unit's call
bool fo_feature_rows(int dtype, int num_levels, const void* const* bases, const long long* cells, const long long* batch_strides,
                     const long long* cell_strides, const long long* channel_strides, int F, int A, int B, long long K,
                     const long long* anchor_index, const void* count, int count_is_int64, FoLevels* L, FoSel* s) {
    return fo_width_ok(F) && A >= 1 && fo_levels(dtype, num_levels, bases, cells, batch_strides, cell_strides, channel_strides, B, L) &&
           fo_sel(B, K, anchor_index, count, count_is_int64, (long long)A * L->P, s);
}
// the class arguments of the ABI -> the kernels' copy; false: refuse
bool fo_classes(const void* classes, int dtype, long long pitch, long long stride, long long offset, int C, FoClasses* c) {
    *c = FoClasses{classes, dtype, pitch, stride, offset, C};
    return classes && dtype >= 0 && dtype <= 2 && pitch >= 0 && stride >= 0;
}

}  // namespace
