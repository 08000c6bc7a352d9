// The accumulate stage that eval_scale.hip (PASCAL-style AP, the open-set counts) and coco_eval.hip (COCO AP / AR, which also
// serves lvis_eval.hip's matches) state once: kept detections are appended to capacity-sized buffers at a cursor
// on the device, sorted by a 48-bit (class, score descending) key with the stable LSD sort of radix_sort.h, and every class
// segment is then walked from the back in chunks of EV_AP_CHUNK entries.  What a unit appends beside (score, class), what
// travels through the sort as payload and its AP kernel stay in the unit.
//
//   append   struct A : EvAppend, with two overloads beside it:
//              bool ev_keep(const A&, long long slot, unsigned* word)               is the slot kept?  *word: the word it read
//              void ev_store(const A&, long long slot, unsigned p, unsigned word)   the slot's payload to position p < capacity;
//                                                                                   word: ev_keep's, so that it is not read again
//            ev_append(stream, a) launches ev_append_write_kernel<A> and ev_append_cursor_kernel.
//   sort     struct S : EvSort with typename S::Item, rs_key (ev_key with the entry's validity), rs_load and rs_store beside it;
//            ev_layout places the buffers in the workspace, ev_sort fills the common fields and launches the passes.
//   AP       ev_live and ev_class_begin, and the two reductions below, called by all EV_THREADS threads of a workgroup.  The walk
//            of a class segment in chunks of EV_AP_CHUNK entries stays in each unit's AP kernel: stated once as a function of a
//            callable here it compiled to slower kernels (profiles/README.md, eval_shared_*).
//
// Both units are compiled with -ffp-contract=off: every float64 term is one division or one addition, one rounding each.
#pragma once
#include "compact.h"
#include "radix_sort.h"
#include "eval_match.h"

namespace {

typedef unsigned long long u64;

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / 64;
static_assert(EV_THREADS == FO_THREADS && EV_THREADS == EM_THREADS, "the shared headers are written for this workgroup size");
constexpr int EV_AP_ITEMS = 8;
constexpr int EV_AP_CHUNK = EV_THREADS * EV_AP_ITEMS;            // segment entries of one AP step (counts fit 16 bits)

// ---- workgroup reductions in a fixed order: all EV_THREADS threads call them; sh: [EV_WAVES] in LDS, free again when the call
// returns.  (The integer scan is fo_block_excl_scan of compact.h.)  ev_block_sum is not fo_block_sum of compact.h: that one is a
// tree over 256 LDS words, this one a butterfly inside a wave and then the waves in ascending order.  Either gives the same bits
// every run, but not the same bits as the other for a float64 sum: ood_eval.hip's AUPR is pinned to the tree, the AP of
// eval_scale.hip to this order, so both stay. ----------------------------------------------------------------------------------
template <typename V> DEV V ev_block_sum(V v, V* sh, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    V tot = sh[0];
#pragma unroll
    for (int w = 1; w < EV_WAVES; ++w) tot = tot + sh[w];
    __syncthreads();
    return tot;
}
// maximum over the threads above this one (0 for the last); *total: over all.  Values are >= 0.
DEV double ev_block_excl_rmax(double v, double* sh, int tid, double* total) {
    const int lane = tid & 63, wave = tid >> 6;
    double incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl = fmax(incl, t);
    }
    const double nxt = __shfl_down(incl, 1, 64);
    double ex = lane < 63 ? nxt : 0.0;
    if (lane == 0) sh[wave] = incl;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) { const double s = sh[w]; if (w > wave) ex = fmax(ex, s); tot = fmax(tot, s); }
    __syncthreads();
    *total = tot;
    return ex;
}

// the live count: n_host, or min(*cursor, capacity) when n_host < 0
DEV unsigned ev_live(const unsigned* cursor, long long n_host, unsigned capacity) {
    return n_host >= 0 ? (unsigned)n_host : fo_min(cursor[0], capacity);
}
// keys[0 .. n) sorted: the first entry of class c (the search of compact.h: the trip count follows from n alone, every read is at
// an index < n).  Class c is the segment [ev_class_begin(c), ev_class_begin(c + 1)).
DEV unsigned ev_class_begin(const u64* keys, unsigned n, int c) {
    const u64 k = (u64)c << 32;
    return fo_partition_point(keys, n, [=](u64 v) { return v < k; });
}

// ---- append ----------------------------------------------------------------------------------------------------------------------
struct EvCursor { const int* kept; int B; unsigned capacity; unsigned* state; };      // kept: [2 B] kept slots, then NaN scores, per image
struct EvAppend {
    const float* det; const int* kept; int B, max_det;
    float* scores; int* classes; unsigned capacity; unsigned* state;                  // state: {cursor, lost, NaN scores, 0}
};

// workgroup b: image b's kept slots, in slot order, from cursor + the kept counts of the images before it
template <typename A> __global__ __launch_bounds__(EV_THREADS) void ev_append_write_kernel(A a) {
    __shared__ unsigned shu[EV_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned before = 0;
    for (int k = tid; k < b; k += EV_THREADS) before += (unsigned)a.kept[k];
    unsigned pos = fo_min(a.state[0], a.capacity) + ev_block_sum<unsigned>(before, shu, tid);
    for (int i0 = 0; i0 < a.max_det; i0 += EV_THREADS) {
        const int i = i0 + tid;
        const long long slot = (long long)b * a.max_det + i;
        unsigned word = 0;
        const bool keep = i < a.max_det && ev_keep(a, slot, &word);
        unsigned total;
        const unsigned p = pos + fo_block_excl_scan(keep ? 1u : 0u, shu, tid, &total);
        if (keep && p < a.capacity) {                                     // beyond the capacity: counted by the cursor launch
            float v = a.det[slot * 6 + 4];
            if (v == 0.f) v = 0.f;                                        // -0.0 is stored as +0.0: the two tie
            a.scores[p] = v;
            a.classes[p] = (int)a.det[slot * 6 + 5] - 1;
            ev_store(a, slot, p, word);
        }
        pos += total;
    }
}

// one workgroup: the cursor moves (clamped to the capacity; the surplus and the NaN scores are counted)
__global__ __launch_bounds__(EV_THREADS) void ev_append_cursor_kernel(EvCursor a) {
    __shared__ unsigned shu[EV_WAVES];
    const int tid = threadIdx.x;
    unsigned kept = 0, nans = 0;
    for (int k = tid; k < a.B; k += EV_THREADS) { kept += (unsigned)a.kept[k]; nans += (unsigned)a.kept[a.B + k]; }
    kept = ev_block_sum<unsigned>(kept, shu, tid);
    nans = ev_block_sum<unsigned>(nans, shu, tid);
    if (tid == 0) {
        const u64 end = (u64)fo_min(a.state[0], a.capacity) + kept;
        if (end > a.capacity) {
            const u64 lost = (u64)a.state[1] + (end - a.capacity);
            a.state[1] = lost > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)lost;
        }
        a.state[0] = end > a.capacity ? a.capacity : (unsigned)end;
        const u64 nn = (u64)a.state[2] + nans;
        a.state[2] = nn > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)nn;
    }
}

template <typename A> int ev_append(void* stream, const A& a) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ev_append_write_kernel<A>, dim3(a.B), dim3(EV_THREADS), 0, st, a);
    hipLaunchKernelGGL(ev_append_cursor_kernel, dim3(1), dim3(EV_THREADS), 0, st, EvCursor{a.kept, a.B, a.capacity, a.state});
    return effdet_check_launch();
}

// ---- sort: what every pass descriptor of radix_sort.h holds here (one problem); the unit adds Item and its payload buffers ---------
struct EvSort {
    typedef u64 Key;
    const float* scores; const int* classes;                              // the first pass reads these
    const u64* src_k; const unsigned* src_v; u64* dst_k; unsigned* dst_v;
    const unsigned* cursor; long long n_host;                             // live count: ev_live
    unsigned* hist; unsigned* totals;
    unsigned capacity, tiles;                                             // tiles by capacity: the row pitch of hist
    int shift, first, C;
};
DEV RsProblem rs_problem(const EvSort& s, unsigned) { return RsProblem{ev_live(s.cursor, s.n_host, s.capacity), s.hist, s.totals, s.tiles}; }
// The key of entry i: after the first pass the one that travels; in the first pass (class << 32) | ~key(score): ascending = class,
// then score descending; -0.0 ties with +0.0.  An entry for which valid(i) does not hold (the unit's own test), of a class
// outside 0..C-1 or with a NaN score gets class C: behind every class.
template <typename Valid> DEV u64 ev_key(const EvSort& s, unsigned i, Valid valid) {
    if (!s.first) return s.src_k[i];
    const bool own = valid(i);
    const int c = s.classes[i];
    float v = s.scores[i];
    const bool ok = own && c >= 0 && c < s.C && v == v;
    if (v == 0.f) v = 0.f;
    return ((u64)(ok ? (unsigned)c : (unsigned)s.C) << 32) | (u64)(~fo_key(__float_as_uint(v)));
}

// ---- workspace layout and the passes (host) ----------------------------------------------------------------------------------------
bool ev_capacity_ok(long long capacity) { return capacity >= 1 && capacity <= EM_MAX_N; }      // entries of a buffer
struct EvLayout { long long keys[2], vals[2], hist, totals, extra[2], total; unsigned tiles; int passes; };

// extra0, extra1: bytes per entry of the unit's own two buffers behind the sort's (0: none, offset 0)
bool ev_layout(long long capacity, int C, long long extra0, long long extra1, EvLayout* L) {
    if (!ev_capacity_ok(capacity) || !em_classes_ok(C)) return false;
    long long off = 0;
    auto take = [&off](long long bytes) { const long long o = off; off += (bytes + 255) & ~255ll; return o; };
    L->tiles = (unsigned)((capacity + RS_TILE - 1) / RS_TILE);
    L->passes = C <= 255 ? 5 : 6;                                         // 4 score digits, then the class (C itself is a key)
    for (int k = 0; k < 2; ++k) { L->keys[k] = take(capacity * 8); L->vals[k] = take(capacity * 4); }
    L->hist = take(256ll * L->tiles * 4);
    L->totals = take(256 * 4);
    L->extra[0] = extra0 ? take(capacity * extra0) : 0;
    L->extra[1] = extra1 ? take(capacity * extra1) : 0;
    L->total = off;
    return true;
}
// the buffers that hold the sorted keys and payload after the last pass
int ev_last(const EvLayout& L) { return (L.passes - 1) & 1; }

// The passes of the sort: entries -> buffers 0 -> 1 -> 0 ...; the grid by n_host, or by the capacity when the count is on the
// device.  s: the unit's descriptor with its own fields set; per_pass(s, d) sets what it has beside keys and vals for a pass into
// buffers d.  -> the grid of a pass (0: nothing was launched).
template <typename S, typename PerPass>
unsigned ev_sort(hipStream_t st, S s, const float* scores, const int* classes, const unsigned* state, long long n_host, long long capacity,
                 int C, char* ws, const EvLayout& L, PerPass per_pass) {
    s.scores = scores; s.classes = classes; s.cursor = state; s.n_host = n_host;
    s.hist = reinterpret_cast<unsigned*>(ws + L.hist); s.totals = reinterpret_cast<unsigned*>(ws + L.totals);
    s.capacity = (unsigned)capacity; s.tiles = L.tiles; s.C = C;
    const unsigned grid = n_host < 0 ? L.tiles : (unsigned)((n_host + RS_TILE - 1) / RS_TILE);
    for (int pass = 0; pass < L.passes && grid > 0; ++pass) {
        const int d = pass & 1;
        s.shift = 8 * pass; s.first = pass == 0;
        s.src_k = reinterpret_cast<const u64*>(ws + L.keys[1 - d]); s.src_v = reinterpret_cast<const unsigned*>(ws + L.vals[1 - d]);
        s.dst_k = reinterpret_cast<u64*>(ws + L.keys[d]); s.dst_v = reinterpret_cast<unsigned*>(ws + L.vals[d]);
        per_pass(s, d);
        rs_sort_pass(st, s, grid, 1);
    }
    return grid;
}

}  // namespace
