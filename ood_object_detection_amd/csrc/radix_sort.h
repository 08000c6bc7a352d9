// One pass of the stable LSD radix sort of ood_eval.hip, outlier_synth.hip and, through eval_sorted.h, eval_scale.hip and
// coco_eval.hip, 8 bits a pass:
//   rs_hist_kernel     workgroup (tile, y): the digit counts of one tile of RS_TILE keys, in LDS by integer atomics -> hist[d][tile]
//   rs_scan_kernel     workgroup (d, y): the exclusive prefix of digit d's counts over the live tiles, in place, and the digit's total
//   rs_scatter_kernel  workgroup (tile, y): every entry of the tile to (digits below in the array) + (this digit in earlier tiles) +
//                      (this digit earlier in the tile); equal digits keep their order
// rs_sort_pass launches the three.  Launch boundaries are the only synchronisation between workgroups, no atomic decides a position,
// every position is compared with the live count before the store, and workgroups beyond the live tiles exit: grids are sized by
// the capacity, the live count is read on the device.
//
// A unit describes a pass by a struct P passed by value, with
//   typename P::Key     unsigned or unsigned long long.  The digit of a pass is (key >> shift) & 255; the padding key of a lane
//                       beyond the live count is all ones
//   typename P::Item    what travels: a member `key` of type Key, and the payload words, if any, beside it
//   int shift
// and four overloads beside it; y = blockIdx.y is the problem of the workgroup (the launches sort `problems` arrays at once):
//   RsProblem rs_problem(const P&, unsigned y)                         the live count, hist, totals and the row pitch of hist
//   Key rs_key(const P&, unsigned y, unsigned i)                       the key of entry i < n: all the histogram reads
//   Item rs_load(const P&, unsigned y, unsigned i)                     entry i < n with its payload
//   void rs_store(const P&, unsigned y, unsigned p, const Item&)       the entry to position p < n of the pass's output
// hist: [256][tiles] unsigned, totals: [256] unsigned, per problem; tiles >= the live tiles.
#pragma once
#include "compact.h"

namespace {

constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = FO_THREADS * RS_ITEMS;                  // keys of one workgroup per pass

struct RsProblem { unsigned n; unsigned* hist; unsigned* totals; unsigned tiles; };

template <typename P> DEV unsigned rs_digit(const P& p, typename P::Key key) { return (unsigned)(key >> p.shift) & 255u; }
DEV unsigned rs_live_tiles(unsigned n) { return (n + RS_TILE - 1) / RS_TILE; }

template <typename P> __global__ __launch_bounds__(256) void rs_hist_kernel(P p) {
    __shared__ unsigned h[256];
    const unsigned y = blockIdx.y, tile = blockIdx.x;
    const RsProblem S = rs_problem(p, y);
    const int tid = threadIdx.x;
    if (tile >= rs_live_tiles(S.n)) return;                     // the same for the whole workgroup
    h[tid] = 0;
    __syncthreads();
    for (int r = 0; r < RS_ITEMS; ++r) {
        const unsigned i = tile * RS_TILE + r * FO_THREADS + tid;
        if (i < S.n) atomicAdd(&h[rs_digit(p, rs_key(p, y, i))], 1u);      // integer counts in LDS: order independent
    }
    __syncthreads();
    S.hist[(unsigned)tid * S.tiles + tile] = h[tid];
}

template <typename P> __global__ __launch_bounds__(256) void rs_scan_kernel(P p) {
    __shared__ unsigned sh[FO_WAVES];
    const RsProblem S = rs_problem(p, blockIdx.y);
    const int tid = threadIdx.x;
    const unsigned ntiles = rs_live_tiles(S.n);
    unsigned* row = S.hist + (unsigned)blockIdx.x * S.tiles;
    const unsigned chunk = (ntiles + FO_THREADS - 1) / FO_THREADS;
    const unsigned lo = fo_min((unsigned)tid * chunk, ntiles), hi = fo_min(lo + chunk, ntiles);
    unsigned sum = 0;
    for (unsigned k = lo; k < hi; ++k) sum += row[k];
    unsigned total;
    unsigned run = fo_block_excl_scan(sum, sh, tid, &total);
    for (unsigned k = lo; k < hi; ++k) { const unsigned c = row[k]; row[k] = run; run += c; }
    if (tid == 0) S.totals[blockIdx.x] = total;
}

// Wave w owns entries [w * 1024, (w + 1) * 1024) of the tile, 64 consecutive ones per round.  An entry's rank among the equal digits
// of its wave = the wave's running count of the digit + the equal digits in lower lanes (ballots); the waves' counts are then
// prefixed per digit on top of (digits below in the array) + (this digit in earlier tiles).
template <typename P> __global__ __launch_bounds__(256) void rs_scatter_kernel(P p) {
    typedef typename P::Key Key;
    typedef typename P::Item Item;
    __shared__ unsigned wcnt[FO_WAVES][256];
    __shared__ unsigned sh[FO_WAVES];
    const unsigned y = blockIdx.y, tile = blockIdx.x;
    const RsProblem S = rs_problem(p, y);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n = S.n;
    if (tile >= rs_live_tiles(n)) return;
    for (int w = 0; w < FO_WAVES; ++w) wcnt[w][tid] = 0;
    unsigned total;
    const unsigned digit_first = fo_block_excl_scan(S.totals[tid], sh, tid, &total) + S.hist[(unsigned)tid * S.tiles + tile];
    // (the scan's barriers also publish the zeroed counters)
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned seg = tile * RS_TILE + (unsigned)wave * (64 * RS_ITEMS);
    Item item[RS_ITEMS];
    unsigned rank[RS_ITEMS];
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const unsigned i = seg + r * 64 + lane;
        const bool valid = i < n;
        item[r] = Item();
        item[r].key = ~(Key)0;
        if (valid) item[r] = rs_load(p, y, i);
        const unsigned d = rs_digit(p, item[r].key);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned lower = fo_popc(same & below);
        const unsigned prev = valid ? wcnt[wave][d] : 0u;
        __builtin_amdgcn_wave_barrier();                        // all lanes of the wave have read the count before one writes it
        if (valid && lower == 0) wcnt[wave][d] = prev + fo_popc(same);     // one lane per digit present in the round
        __builtin_amdgcn_wave_barrier();
        rank[r] = prev + lower;
    }
    __syncthreads();
    {   // thread d: the waves' counts of digit d -> first positions
        unsigned run = digit_first;
        for (int w = 0; w < FO_WAVES; ++w) { const unsigned c = wcnt[w][tid]; wcnt[w][tid] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const unsigned i = seg + r * 64 + lane;
        if (i < n) {
            const unsigned pos = wcnt[wave][rs_digit(p, item[r].key)] + rank[r];
            if (pos < n) rs_store(p, y, pos, item[r]);
        }
    }
}

// one pass over `problems` arrays of at most tiles * RS_TILE live entries each
template <typename P> void rs_sort_pass(hipStream_t st, const P& p, unsigned tiles, unsigned problems) {
    hipLaunchKernelGGL(rs_hist_kernel<P>, dim3(tiles, problems), dim3(FO_THREADS), 0, st, p);
    hipLaunchKernelGGL(rs_scan_kernel<P>, dim3(256, problems), dim3(FO_THREADS), 0, st, p);
    hipLaunchKernelGGL(rs_scatter_kernel<P>, dim3(tiles, problems), dim3(FO_THREADS), 0, st, p);
}

}  // namespace
