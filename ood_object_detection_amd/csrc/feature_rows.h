// Row addressing of the feature-space OOD units (feature_ood.hip, feature_knn.hip): rows are F-vectors of pyramid cells, read through
// a level table (<= 8 entries: base, cells, batch stride, cell stride; channel stride 1), float32 or bfloat16; and the workgroup
// reductions of their valid-row compaction (counts -> bases -> writes, 2048 [B, K] entries per workgroup of 256 threads).
#pragma once
#include "common.h"

namespace {

constexpr int FO_THREADS = 256;
constexpr int FO_ITEMS = 8;
constexpr int FO_TILE = FO_THREADS * FO_ITEMS;                  // [B, K] entries of one compaction workgroup
constexpr long long FO_MAX_ROWS = 1ll << 27;                    // B * K of one call
constexpr long long FO_MAX_BLOCKS = FO_MAX_ROWS / FO_TILE;
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

DEV unsigned fo_min(unsigned a, unsigned b) { return a < b ? a : b; }
DEV unsigned fo_popc(unsigned long long m) { return (unsigned)__builtin_popcountll(m); }

template <typename T> DEV T fo_block_sum(T v, T* sh, int tid) {
    sh[tid] = v;
    __syncthreads();
    for (int s = FO_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}
DEV unsigned fo_block_excl_scan(unsigned v, unsigned* sh, int tid, unsigned* total) {
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < FO_THREADS; off <<= 1) {
        const unsigned t = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const unsigned incl = sh[tid];
    *total = sh[FO_THREADS - 1];
    __syncthreads();
    return incl - v;
}

DEV long long fo_count(const void* count, int is64, unsigned b) {
    return is64 ? reinterpret_cast<const long long*>(count)[b] : (long long)reinterpret_cast<const int*>(count)[b];
}

// ---- host ----
bool fo_width_ok(int F) { return F == 64 || F == 88 || F == 112 || F == 160 || F == 224 || F == 288; }

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

}  // namespace
