// Workgroup reductions, integer helpers, the workspace carve and the ordered compaction that the OOD and the evaluation units share (feature_ood.hip,
// feature_knn.hip, feature_subspace.hip, logit_ood.hip, act_shaping.hip, energy_reg.hip, outlier_synth.hip, ood_eval.hip, and through radix_sort.h,
// eval_match.h and eval_sorted.h the evaluation units eval_scale.hip, coco_eval.hip, lvis_eval.hip).  The compaction: the kept entries of a [B, K] call
// get consecutive positions in (b, j) order by three launches - kept entries per tile of 2048 (fo_count_kernel), the tiles' first
// positions in one workgroup (fo_base_kernel), then ballot ranks inside a tile (fo_positions, called by the unit's own write
// kernel, or by fo_write_index_kernel where the list holds the entry index).  No atomic decides a position.  A unit describes its compaction by a struct
// A with `unsigned* counts` ([nblocks]), `unsigned nblocks` and three overloads beside it:
//   bool cp_keep(const A&, unsigned i)                          is entry i kept?  (false at i >= total)
//   unsigned cp_begin(const A&)                                 the position of the first kept entry
//   void cp_finish(const A&, unsigned begin, unsigned total)    thread 0 of the base workgroup: publish the number of kept entries
#pragma once
#include "common.h"

namespace {

constexpr int FO_THREADS = 256;
constexpr int FO_WAVES = FO_THREADS / 64;
constexpr int FO_ITEMS = 8;
constexpr int FO_TILE = FO_THREADS * FO_ITEMS;                  // [B, K] entries of one compaction workgroup

DEV unsigned fo_min(unsigned a, unsigned b) { return a < b ? a : b; }
DEV unsigned fo_popc(unsigned long long m) { return (unsigned)__builtin_popcountll(m); }
// float32 bits -> key whose unsigned order is the order of the floats, and back
DEV unsigned fo_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
DEV unsigned fo_unkey(unsigned key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }
// largest power of two <= n (0 for 0)
DEV unsigned fo_floor_pow2(unsigned n) {
    n |= n >> 1; n |= n >> 2; n |= n >> 4; n |= n >> 8; n |= n >> 16;
    return n - (n >> 1);
}
// a[0 .. n) is ordered so that the entries for which `before` holds come first: their number.  Branch-free binary search: the trip
// count follows from n alone, and every read is at an index < n.
template <typename T, typename Before> DEV unsigned fo_partition_point(const T* a, unsigned n, Before before) {
    unsigned lo = 0;
    for (unsigned step = fo_floor_pow2(n); step > 0; step >>= 1) {
        const unsigned nxt = lo + step;
        if (nxt <= n && before(a[nxt - 1])) lo = nxt;
    }
    return lo;
}

// All FO_THREADS threads call it; sh: [FO_THREADS] of T in LDS.  Fixed order (a tree), so a float64 sum has the same bits every run.
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
// Exclusive prefix of v over the threads, *total: the sum over all.  All FO_THREADS threads call it; sh: [FO_WAVES] in LDS, free again
// when the call returns.  Shuffles inside a wave, then the waves in order: two barriers.  Integers only, so any order gives the same.
DEV unsigned fo_block_excl_scan(unsigned v, unsigned* sh, int tid, unsigned* total) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    unsigned before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < FO_WAVES; ++w) { const unsigned s = sh[w]; before += w < wave ? s : 0u; tot += s; }
    __syncthreads();
    *total = tot;
    return before + incl - v;
}

template <typename A> __global__ __launch_bounds__(256) void fo_count_kernel(A a) {
    __shared__ unsigned sh[FO_THREADS];
    const int tid = threadIdx.x;
    const unsigned base = (unsigned)blockIdx.x * FO_TILE;
    unsigned c = 0;
    for (int r = 0; r < FO_ITEMS; ++r) c += cp_keep(a, base + r * FO_THREADS + tid) ? 1u : 0u;
    const unsigned tot = fo_block_sum<unsigned>(c, sh, tid);
    if (tid == 0) a.counts[blockIdx.x] = tot;
}

// one workgroup: counts -> first positions of the workgroups
template <typename A> __global__ __launch_bounds__(256) void fo_base_kernel(A a) {
    __shared__ unsigned sh[FO_WAVES];
    const int tid = threadIdx.x;
    const unsigned begin = cp_begin(a);
    const unsigned chunk = (a.nblocks + FO_THREADS - 1) / FO_THREADS;
    const unsigned lo = fo_min((unsigned)tid * chunk, a.nblocks), hi = fo_min(lo + chunk, a.nblocks);
    unsigned sum = 0;
    for (unsigned k = lo; k < hi; ++k) sum += a.counts[k];
    unsigned total;
    unsigned run = begin + fo_block_excl_scan(sum, sh, tid, &total);
    for (unsigned k = lo; k < hi; ++k) { const unsigned c = a.counts[k]; a.counts[k] = run; run += c; }
    if (tid == 0) cp_finish(a, begin, total);                   // the scan's barriers order what cp_begin read before what this writes
}

// entry r (< FO_ITEMS) of this lane in a write kernel: wave w of a workgroup owns entries [w * 512, (w + 1) * 512) of its tile, 64
// consecutive ones per round, so positions follow (b, j)
DEV unsigned fo_entry(int r) {
    return (unsigned)blockIdx.x * FO_TILE + (threadIdx.x >> 6) * (64 * FO_ITEMS) + r * 64 + (threadIdx.x & 63);
}
// The write step, called by all FO_THREADS threads of workgroup blockIdx.x: bit r of the result says whether keep(r, fo_entry(r))
// held, and pos[r] is then the entry's position (counts: the bases fo_base_kernel left).  The caller compares it with its capacity.
template <typename Keep> DEV unsigned fo_positions(const unsigned* counts, unsigned (&pos)[FO_ITEMS], Keep keep) {
    __shared__ unsigned wsum[FO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned kept = 0, wtot = 0;
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r) {
        const bool k = keep(r, fo_entry(r));
        const unsigned long long bal = __ballot(k);
        pos[r] = wtot + fo_popc(bal & below);
        wtot += fo_popc(bal);
        kept |= (k ? 1u : 0u) << r;
    }
    if (lane == 0) wsum[wave] = wtot;
    __syncthreads();
    unsigned first = counts[blockIdx.x];
    for (int w = 0; w < FO_THREADS / 64; ++w) first += w < wave ? wsum[w] : 0u;
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r) pos[r] += first;
    return kept;
}

// The write kernel of a unit whose compacted list holds the entry index itself (logit_ood.hip, act_shaping.hip): A has beside
// `counts` an `unsigned* list` of `sel.total` places.  The three overloads stay the unit's own: a template of them here would
// stand in for an overload that a unit forgot.
template <typename A> __global__ __launch_bounds__(256) void fo_write_index_kernel(A a) {
    unsigned pos[FO_ITEMS];
    const unsigned kept = fo_positions(a.counts, pos, [&](int, unsigned i) { return cp_keep(a, i); });
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r)
        if ((kept & (1u << r)) && pos[r] < a.sel.total) a.list[pos[r]] = fo_entry(r);
}

// ---- host ----
// Carves a workspace: take(bytes) is the offset of the next region, every region a multiple of 256 bytes; `at` the bytes taken so far
struct FoCarve {
    long long at = 0;
    long long take(long long bytes) { const long long o = at; at += (bytes + 255) & ~255ll; return o; }
};

}  // namespace
