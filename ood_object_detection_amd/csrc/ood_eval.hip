// Detection-level OOD evaluation on the device: AUROC pair counts, AUPR (in / out) and FPR at a TPR level over two multisets of
// float32 scores, `pos` (in-distribution, P values) and `neg` (OOD, N values); a higher score means more in-distribution.
//
//   append   [B, K] score matrix -> one side's flat buffer, in (b, j) order from a cursor that lives on the device: the ordered
//            compaction of compact.h, whose base launch also moves the cursor.  No atomic decides a position.
//   sort     both sides through the same launches (a two-entry problem table, blockIdx.y = side): the LSD radix sort of
//            radix_sort.h over the 32-bit order-preserving keys, four passes, no payload.
//   metrics  everything follows from the two sorted arrays by binary search: one launch of per-workgroup partials (uint64 pair
//            counts, float64 AUPR terms), one workgroup that adds them in a fixed order and fills the result block.
//
// Launch boundaries are the only synchronisation between workgroups.  Every loop has a trip count known at its entry, every
// scatter index is compared with the segment length before the store, and the element counts are read from the device cursors
// (grids are sized by the capacities; workgroups beyond the live count exit), so the host never reads anything back.
#include "common.h"
#include "compact.h"
#include "radix_sort.h"

namespace {

typedef unsigned long long u64;

constexpr int OE_THREADS = 256;
static_assert(OE_THREADS == FO_THREADS, "the reductions, the compaction and the sort of the shared headers are written for this workgroup size");
constexpr int OE_MET_ITEMS = 8;
constexpr int OE_MET_TILE = OE_THREADS * OE_MET_ITEMS;            // sorted scores of one workgroup
constexpr long long OE_MAX_SCORES = 1ll << 27;                    // per side, and per append call
constexpr long long OE_APPEND_MAX_BLOCKS = OE_MAX_SCORES / FO_TILE;   // FO_TILE matrix entries per append workgroup

// flag bits of a side's state word 1, and of the result block
constexpr unsigned OE_SIDE_NAN = 1u, OE_SIDE_OVERFLOW = 2u;
constexpr unsigned OE_RES_EMPTY_IN = 16u, OE_RES_EMPTY_OOD = 32u;

// ---- workspace layout (host) -------------------------------------------------------------------------------------------------
struct OeLayout {
    long long append_counts;                    // [OE_APPEND_MAX_BLOCKS] unsigned: kept entries per append workgroup, then bases
    long long keys_a[2], keys_b[2];             // [capacity] unsigned each; the sorted float32 scores end in keys_b
    long long hist[2];                          // [256][tiles] unsigned: digit counts per tile, then exclusive tile prefixes
    long long totals[2];                        // [256] unsigned: digit totals of the pass
    long long part_gt[2], part_eq[2], part_ap[2];   // [metric blocks] partials
    long long total;
    unsigned tiles[2], mblocks[2];
};

bool oe_layout(long long cap_pos, long long cap_neg, OeLayout* L) {
    if (cap_pos < 1 || cap_neg < 1 || cap_pos > OE_MAX_SCORES || cap_neg > OE_MAX_SCORES) return false;
    long long off = 0;
    auto take = [&off](long long bytes) { const long long o = off; off += (bytes + 255) & ~255ll; return o; };
    L->append_counts = take(OE_APPEND_MAX_BLOCKS * 4);
    const long long caps[2] = {cap_pos, cap_neg};
    for (int s = 0; s < 2; ++s) {
        L->tiles[s] = (unsigned)((caps[s] + RS_TILE - 1) / RS_TILE);
        L->mblocks[s] = (unsigned)((caps[s] + OE_MET_TILE - 1) / OE_MET_TILE);
        L->keys_a[s] = take(caps[s] * 4);
        L->keys_b[s] = take(caps[s] * 4);
        L->hist[s] = take(256ll * L->tiles[s] * 4);
        L->totals[s] = take(256 * 4);
        L->part_gt[s] = take((long long)L->mblocks[s] * 8);
        L->part_eq[s] = take((long long)L->mblocks[s] * 8);
        L->part_ap[s] = take((long long)L->mblocks[s] * 8);
    }
    L->total = off;
    return true;
}

// a[0 .. n) holds float32 bits in ascending order: the number of entries whose key is < k (upper == 0) or <= k (upper != 0), by
// the search of compact.h: the trip count follows from n alone, and every read is at an index < n
DEV unsigned oe_bound(const unsigned* a, unsigned n, unsigned k, int upper) {
    return fo_partition_point(a, n, [=](unsigned bits) { const unsigned v = fo_key(bits); return upper ? v <= k : v < k; });
}

// ---- append ------------------------------------------------------------------------------------------------------------------
struct OeAppend {
    const float* scores; long long pitch, stride;
    const void* count; int count_i64;
    const float* det; long long det_pitch, det_stride; float min_score;
    int negate, K;
    unsigned total;                             // B * K
    float* buffer; unsigned capacity;
    unsigned* state;                            // the side's {cursor, flags}
    unsigned* counts; unsigned nblocks;
};

// is entry i = b * K + j kept?  src: its offset in `scores`
DEV bool oe_keep(const OeAppend& a, unsigned i, long long* src) {
    if (i >= a.total) return false;
    const unsigned b = i / (unsigned)a.K, j = i - b * (unsigned)a.K;
    if (a.count) {
        const long long c = a.count_i64 ? reinterpret_cast<const long long*>(a.count)[b] : (long long)reinterpret_cast<const int*>(a.count)[b];
        if ((long long)j >= c) return false;
    }
    if (a.det && !(a.det[(long long)b * a.det_pitch + (long long)j * a.det_stride] >= a.min_score)) return false;
    *src = (long long)b * a.pitch + (long long)j * a.stride;
    return true;
}

DEV bool cp_keep(const OeAppend& a, unsigned i) { long long src; return oe_keep(a, i, &src); }
// positions start at the cursor (clamped to the capacity).  fo_base_kernel reads it here, before the barriers of its scan, and
// calls cp_finish after them: the barriers order the read of the cursor before its write
DEV unsigned cp_begin(const OeAppend& a) { return fo_min(a.state[0], a.capacity); }
// the cursor moves (clamped to the capacity, overflow flagged)
DEV void cp_finish(const OeAppend& a, unsigned c0, unsigned total) {
    const u64 end = (u64)c0 + total;
    if (end > a.capacity) a.state[1] |= OE_SIDE_OVERFLOW;
    a.state[0] = end > a.capacity ? a.capacity : (unsigned)end;
}

__global__ __launch_bounds__(256) void oe_append_write_kernel(OeAppend a) {
    long long src[FO_ITEMS];
    unsigned pos[FO_ITEMS];
    const unsigned kept = fo_positions(a.counts, pos, [&](int r, unsigned i) {
        src[r] = 0;
        return oe_keep(a, i, &src[r]);
    });
    bool nan = false;
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r) {
        if (kept & (1u << r)) {
            float v = a.scores[src[r]];
            if (a.negate) v = -v;
            if (v != v) nan = true;
            if (v == 0.f) v = 0.f;                                      // -0.0 is stored as +0.0: the two tie
            if (pos[r] < a.capacity) a.buffer[pos[r]] = v;              // beyond the capacity: dropped (the base launch set the flag)
        }
    }
    if (nan) atomicOr(&a.state[1], OE_SIDE_NAN);                        // an OR of a flag bit: no order to depend on
}

// ---- sort: the pass descriptor of radix_sort.h --------------------------------------------------------------------------------
struct OeSortSide {
    const unsigned* src; unsigned* dst;
    const unsigned* cursor;                     // live count = min(*cursor, capacity)
    unsigned* hist; unsigned* totals;
    unsigned capacity, tiles;                   // tiles by capacity: the row pitch of hist
};
struct OeItem { unsigned key; };               // keys only: every metric is a function of the two sorted multisets
struct OeSort {
    typedef unsigned Key;
    typedef OeItem Item;
    OeSortSide s[2];
    int shift, first, last;                     // first: src holds float bits; last: dst receives float bits
};

DEV RsProblem rs_problem(const OeSort& t, unsigned side) {
    const OeSortSide& S = t.s[side];
    return RsProblem{fo_min(S.cursor[0], S.capacity), S.hist, S.totals, S.tiles};
}
DEV unsigned rs_key(const OeSort& t, unsigned side, unsigned i) {
    const unsigned v = t.s[side].src[i];
    return t.first ? fo_key(v) : v;
}
DEV OeItem rs_load(const OeSort& t, unsigned side, unsigned i) { return OeItem{rs_key(t, side, i)}; }
DEV void rs_store(const OeSort& t, unsigned side, unsigned p, const OeItem& e) { t.s[side].dst[p] = t.last ? fo_unkey(e.key) : e.key; }

// ---- metrics -----------------------------------------------------------------------------------------------------------------
struct OeMetrics {
    const unsigned* sorted[2];                  // float32 bits, ascending
    const unsigned* state;                      // {cursor, flags} of pos, then of neg
    unsigned capacity[2];
    u64* part_gt[2]; u64* part_eq[2]; double* part_ap[2];
    double level;
    u64* result;
};

// blockIdx.y = 0: the positives' shares of pairs_gt / pairs_eq and the terms of aupr_in; 1: the terms of aupr_out
__global__ __launch_bounds__(256) void oe_metrics_part_kernel(OeMetrics m) {
    __shared__ u64 shu[OE_THREADS];
    __shared__ double shd[OE_THREADS];
    const int tid = threadIdx.x, side = blockIdx.y;
    const unsigned P = fo_min(m.state[0], m.capacity[0]), N = fo_min(m.state[2], m.capacity[1]);
    const unsigned n_own = side == 0 ? P : N, n_other = side == 0 ? N : P;
    if (P == 0 || N == 0 || (unsigned)blockIdx.x * OE_MET_TILE >= n_own) return;
    const unsigned* own = m.sorted[side];
    const unsigned* other = m.sorted[1 - side];
    u64 gt = 0, eq = 0;
    double ap = 0.0;
    for (int r = 0; r < OE_MET_ITEMS; ++r) {
        const unsigned i = (unsigned)blockIdx.x * OE_MET_TILE + r * OE_THREADS + tid;
        if (i < n_own) {
            const unsigned k = fo_key(own[i]);
            const bool group_end = i + 1 == n_own || fo_key(own[i + 1]) != k;
            if (side == 0) {
                const unsigned lb = oe_bound(other, n_other, k, 0), ub = oe_bound(other, n_other, k, 1);
                gt += lb; eq += ub - lb;
                if (group_end) {
                    const unsigned first = oe_bound(own, n_own, k, 0);
                    const unsigned c = i + 1 - first, tp = n_own - first, fp = n_other - lb;
                    ap += ((double)c / (double)P) * ((double)tp / (double)((u64)tp + fp));
                }
            } else if (group_end) {
                const unsigned first = oe_bound(own, n_own, k, 0);
                const unsigned c = i + 1 - first, le_own = i + 1, le_other = oe_bound(other, n_other, k, 1);
                ap += ((double)c / (double)N) * ((double)le_own / (double)((u64)le_own + le_other));
            }
        }
    }
    gt = fo_block_sum<u64>(gt, shu, tid);
    eq = fo_block_sum<u64>(eq, shu, tid);
    ap = fo_block_sum<double>(ap, shd, tid);
    if (tid == 0) { m.part_gt[side][blockIdx.x] = gt; m.part_eq[side][blockIdx.x] = eq; m.part_ap[side][blockIdx.x] = ap; }
}

// one workgroup: the partials in a fixed order, the operating point at the TPR level, the result block
__global__ __launch_bounds__(256) void oe_metrics_final_kernel(OeMetrics m) {
    __shared__ u64 shu[OE_THREADS];
    __shared__ double shd[OE_THREADS];
    const int tid = threadIdx.x;
    const unsigned P = fo_min(m.state[0], m.capacity[0]), N = fo_min(m.state[2], m.capacity[1]);
    const bool empty = P == 0 || N == 0;
    const unsigned nb0 = empty ? 0u : (P + OE_MET_TILE - 1) / OE_MET_TILE, nb1 = empty ? 0u : (N + OE_MET_TILE - 1) / OE_MET_TILE;
    u64 gt = 0, eq = 0;
    double ap_in = 0.0, ap_out = 0.0;
    for (unsigned k = tid; k < nb0; k += OE_THREADS) { gt += m.part_gt[0][k]; eq += m.part_eq[0][k]; ap_in += m.part_ap[0][k]; }
    for (unsigned k = tid; k < nb1; k += OE_THREADS) ap_out += m.part_ap[1][k];
    gt = fo_block_sum<u64>(gt, shu, tid);
    eq = fo_block_sum<u64>(eq, shu, tid);
    ap_in = fo_block_sum<double>(ap_in, shd, tid);
    ap_out = fo_block_sum<double>(ap_out, shd, tid);
    if (tid != 0) return;
    u64 flags = (u64)(m.state[1] & 3u) | ((u64)(m.state[3] & 3u) << 2);
    if (P == 0) flags |= OE_RES_EMPTY_IN;
    if (N == 0) flags |= OE_RES_EMPTY_OOD;
    u64 tp = 0, fp = 0, rank = 0;
    unsigned thr = 0;
    if (!empty) {
        // the smallest k with (double)k / (double)P >= level: level * P rounds once, so the candidate is off by one at the most
        const double dp = (double)P;
        long long k = (long long)ceil(m.level * dp);
        if (k < 1) k = 1;
        if (k > (long long)P) k = P;
        for (int s = 0; s < 2; ++s) if (k > 1 && (double)(k - 1) / dp >= m.level) --k;
        for (int s = 0; s < 2; ++s) if (k < (long long)P && (double)k / dp < m.level) ++k;
        rank = (u64)k;
        thr = m.sorted[0][P - (unsigned)k];                             // the k-th largest positive
        const unsigned key = fo_key(thr);
        tp = P - oe_bound(m.sorted[0], P, key, 0);
        fp = N - oe_bound(m.sorted[1], N, key, 0);
    }
    u64* res = m.result;
    res[0] = P; res[1] = N; res[2] = gt; res[3] = eq; res[4] = tp; res[5] = fp; res[6] = flags; res[7] = rank;
    reinterpret_cast<double*>(res)[8] = ap_in;
    reinterpret_cast<double*>(res)[9] = ap_out;
    res[10] = (u64)thr;                                                 // float32 bits of the threshold in the low word
    res[11] = 0;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" int effdet_ood_eval_sort_tile(void) { return RS_TILE; }

extern "C" long long effdet_ood_eval_workspace_bytes(long long capacity_pos, long long capacity_neg) {
    OeLayout L;
    return oe_layout(capacity_pos, capacity_neg, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_ood_eval_sorted_offset(long long capacity_pos, long long capacity_neg, int side) {
    OeLayout L;
    if ((side != 0 && side != 1) || !oe_layout(capacity_pos, capacity_neg, &L)) return EFFDET_EINVAL;
    return L.keys_b[side];
}

extern "C" int effdet_ood_eval_append(void* stream, const float* scores, long long pitch, long long stride, int B, int K,
                                      const void* count, int count_is_int64, const float* det_score, long long det_pitch,
                                      long long det_stride, float min_score, int negate, float* buffer, long long capacity,
                                      unsigned int* side_state, void* workspace, long long workspace_bytes) {
    EFFDET_ENTER();
    if (!scores || !buffer || !side_state || !workspace || B <= 0 || K <= 0 || pitch < 0 || stride < 0 || det_pitch < 0 || det_stride < 0)
        return EFFDET_EINVAL;
    if (capacity < 1 || capacity > OE_MAX_SCORES || (long long)B * K > OE_MAX_SCORES || workspace_bytes < OE_APPEND_MAX_BLOCKS * 4)
        return EFFDET_EINVAL;
    OeAppend a;
    a.scores = scores; a.pitch = pitch; a.stride = stride;
    a.count = count; a.count_i64 = count_is_int64 ? 1 : 0;
    a.det = det_score; a.det_pitch = det_pitch; a.det_stride = det_stride; a.min_score = min_score;
    a.negate = negate ? 1 : 0; a.K = K;
    a.total = (unsigned)((long long)B * K);
    a.buffer = buffer; a.capacity = (unsigned)capacity;
    a.state = side_state;
    a.counts = reinterpret_cast<unsigned*>(workspace);                  // OeLayout::append_counts is the head of the workspace
    a.nblocks = (a.total + FO_TILE - 1) / FO_TILE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fo_count_kernel<OeAppend>, dim3(a.nblocks), dim3(OE_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_base_kernel<OeAppend>, dim3(1), dim3(OE_THREADS), 0, st, a);
    hipLaunchKernelGGL(oe_append_write_kernel, dim3(a.nblocks), dim3(OE_THREADS), 0, st, a);
    return effdet_check_launch();
}

extern "C" int effdet_ood_eval_sort(void* stream, const float* pos, long long capacity_pos, const float* neg, long long capacity_neg,
                                    const unsigned int* state, void* workspace, long long workspace_bytes) {
    EFFDET_ENTER();
    OeLayout L;
    if (!pos || !neg || !state || !workspace || !oe_layout(capacity_pos, capacity_neg, &L) || workspace_bytes < L.total) return EFFDET_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    const float* in[2] = {pos, neg};
    const long long caps[2] = {capacity_pos, capacity_neg};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid_x = L.tiles[0] > L.tiles[1] ? L.tiles[0] : L.tiles[1];
    for (int pass = 0; pass < 4; ++pass) {
        OeSort t;
        t.shift = 8 * pass; t.first = pass == 0; t.last = pass == 3;
        for (int s = 0; s < 2; ++s) {
            unsigned* a = reinterpret_cast<unsigned*>(ws + L.keys_a[s]);
            unsigned* b = reinterpret_cast<unsigned*>(ws + L.keys_b[s]);
            t.s[s].src = pass == 0 ? reinterpret_cast<const unsigned*>(in[s]) : (pass & 1) ? a : b;      // in -> a -> b -> a -> b
            t.s[s].dst = (pass & 1) ? b : a;
            t.s[s].cursor = state + 2 * s;
            t.s[s].hist = reinterpret_cast<unsigned*>(ws + L.hist[s]);
            t.s[s].totals = reinterpret_cast<unsigned*>(ws + L.totals[s]);
            t.s[s].capacity = (unsigned)caps[s];
            t.s[s].tiles = L.tiles[s];
        }
        rs_sort_pass(st, t, grid_x, 2);
    }
    return effdet_check_launch();
}

extern "C" int effdet_ood_eval_metrics(void* stream, long long capacity_pos, long long capacity_neg, const unsigned int* state,
                                       void* workspace, long long workspace_bytes, double level, void* result) {
    EFFDET_ENTER();
    OeLayout L;
    if (!state || !workspace || !result || !oe_layout(capacity_pos, capacity_neg, &L) || workspace_bytes < L.total) return EFFDET_EINVAL;
    if (!(level > 0.0 && level <= 1.0)) return EFFDET_EINVAL;
    char* ws = reinterpret_cast<char*>(workspace);
    OeMetrics m;
    for (int s = 0; s < 2; ++s) {
        m.sorted[s] = reinterpret_cast<const unsigned*>(ws + L.keys_b[s]);
        m.part_gt[s] = reinterpret_cast<u64*>(ws + L.part_gt[s]);
        m.part_eq[s] = reinterpret_cast<u64*>(ws + L.part_eq[s]);
        m.part_ap[s] = reinterpret_cast<double*>(ws + L.part_ap[s]);
    }
    m.state = state;
    m.capacity[0] = (unsigned)capacity_pos; m.capacity[1] = (unsigned)capacity_neg;
    m.level = level;
    m.result = reinterpret_cast<u64*>(result);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid_x = L.mblocks[0] > L.mblocks[1] ? L.mblocks[0] : L.mblocks[1];
    hipLaunchKernelGGL(oe_metrics_part_kernel, dim3(grid_x, 2), dim3(OE_THREADS), 0, st, m);
    hipLaunchKernelGGL(oe_metrics_final_kernel, dim3(1), dim3(OE_THREADS), 0, st, m);
    return effdet_check_launch();
}
