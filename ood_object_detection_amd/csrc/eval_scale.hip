// Dataset-scale detection evaluation on the device: the PASCAL-style AP / CorLoc of evaluation.hip for a whole validation set, at
// up to 16 IoU thresholds in one pass.  Compiled with -ffp-contract=off: IoU must round like the reference's separate float32 numpy
// operations (effdet/evaluation/np_box_ops.py), and every float64 term of AP is a division, a subtraction, a product, one rounding each.
//
//   match    one workgroup per image, as eval_match_kernel: detections in descending score order, each takes the ground-truth box of
//            its class with the largest IoU (first on ties; `difficult` boxes take part).  That candidate does not depend on the
//            threshold, so one serial walk serves all T thresholds: a T-bit `taken` mask per box; a detection whose candidate is
//            difficult is IGNORED at the thresholds its IoU reaches (per_image_evaluation.py:391-407, :471).  One flag word per slot.
//   append   (score, class, flag word) of the valid slots -> capacity-sized buffers at a cursor that lives on the device, in (image,
//            slot) order: the images' kept counts come from the match launch, a workgroup adds up the counts of the images before
//            its own, a one-workgroup launch moves the cursor.  No atomic decides a position.
//   sort     stable LSD radix sort of 48-bit keys (class, then score descending) with the flag word as payload, 8 bits a pass, every
//            pass = histogram launch, scan launch, stable scatter launch (the structure of ood_eval.hip).  Equal scores keep their
//            arrival order; every class is one contiguous segment; invalid entries sort behind the last class.
//   AP       one workgroup per (class, threshold) over its segment: the totals first, then the 2048-entry chunks from the last to the
//            first: rank and cumulative TP by an integer scan, precision = ctp / rank in float64, the VOC envelope by a reverse
//            max-scan carried from chunk to chunk (a maximum: exact), AP = sum over the true positives of (recall step) * envelope
//            in a fixed order.  No floating-point atomics; the same sorted input gives the same bits.
//   open     the open-set protocol on the same pipeline, the last class being "unknown": an open word per kept known-class
//            detection (bit t: its largest IoU with the image's unknown boxes reaches threshold t) travels through the append and the
//            sort as a second payload word; after the same AP launch one workgroup per (class, threshold) counts detections, true
//            positives and open detections, in total and up to the position at which recall is nearest a level (integers only).
//            A one-launch kernel relabels detections below a score threshold as unknown.
//
// Launch boundaries are the only synchronisation between workgroups.  Every loop has a trip count known at its entry, every scatter
// index is compared with the live count before the store; the live count is read from the device cursor (grids are sized by the
// capacity; workgroups beyond the live count exit), so the host never reads anything back.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int ES_THREADS = 256;
constexpr int ES_WAVES = ES_THREADS / 64;
constexpr int ES_SORT_ITEMS = 16;
constexpr int ES_SORT_TILE = ES_THREADS * ES_SORT_ITEMS;          // keys of one workgroup per pass
constexpr int ES_AP_ITEMS = 8;
constexpr int ES_AP_CHUNK = ES_THREADS * ES_AP_ITEMS;             // segment entries of one AP step (counts fit 16 bits)
constexpr long long ES_MAX_N = 1ll << 24;
constexpr int ES_MAX_T = 16, ES_MAX_C = 65535;
constexpr unsigned ES_INVALID = 0x80000000u;
constexpr int ES_RESULT_HEAD = 8;                                 // 8-byte words before the AP matrix

DEV unsigned es_min(unsigned a, unsigned b) { return a < b ? a : b; }
DEV unsigned es_popc(u64 m) { return (unsigned)__builtin_popcountll(m); }
// float32 bits -> key whose unsigned order is the order of the floats
DEV unsigned es_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
DEV unsigned es_floor_pow2(unsigned n) {
    n |= n >> 1; n |= n >> 2; n |= n >> 4; n |= n >> 8; n |= n >> 16;
    return n - (n >> 1);
}
// a[0 .. n) ascending: the number of entries < k.  The trip count follows from n alone, every read is at an index < n.
DEV unsigned es_lower_bound(const u64* a, unsigned n, u64 k) {
    unsigned lo = 0;
    for (unsigned step = es_floor_pow2(n); step > 0; step >>= 1) {
        const unsigned nxt = lo + step;
        if (nxt <= n && a[nxt - 1] < k) lo = nxt;
    }
    return lo;
}

// ---- workgroup scans: all ES_THREADS threads call them; sh: [ES_WAVES] in LDS, free again when the call returns -----------------
DEV unsigned es_block_excl_scan(unsigned v, unsigned* sh, int tid, unsigned* total) {
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
    for (int w = 0; w < ES_WAVES; ++w) { const unsigned s = sh[w]; before += w < wave ? s : 0u; tot += s; }
    __syncthreads();
    *total = tot;
    return before + incl - v;
}
// sum in a fixed order (butterfly inside a wave, then the waves in order): the same bits every run
template <typename V> DEV V es_block_sum(V v, V* sh, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    V tot = sh[0];
#pragma unroll
    for (int w = 1; w < ES_WAVES; ++w) tot = tot + sh[w];
    __syncthreads();
    return tot;
}
// maximum over the threads above this one (0 for the last); *total: over all.  Values are >= 0.
DEV double es_block_excl_rmax(double v, double* sh, int tid, double* total) {
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
    for (int w = 0; w < ES_WAVES; ++w) { const double s = sh[w]; if (w > wave) ex = fmax(ex, s); tot = fmax(tot, s); }
    __syncthreads();
    *total = tot;
    return ex;
}

// ---- matching --------------------------------------------------------------------------------------------------------------------
struct EsMatch {
    const float* det; const int* det_count; const float* gt_boxes; const long long* gt_cls; const unsigned char* gt_difficult;
    int B, max_det, M, C, T; float thr[ES_MAX_T];
    unsigned* flags; int* kept; int* gt_count; int* gt_imgs; int* correct;
};

__global__ __launch_bounds__(ES_THREADS) void es_match_kernel(EsMatch p) {
    extern __shared__ int sh[];
    int* seen = sh;                                  // [C] class already had its top-scoring detection
    int* taken = sh + p.C;                           // [M] bit t: taken at threshold t
    int* gcls = taken + p.M;                         // [M] 0-based class or -1
    int* gdif = gcls + p.M;                          // [M]
    float* red_v = reinterpret_cast<float*>(gdif + p.M);    // [4]
    int* red_i = reinterpret_cast<int*>(red_v + 4);          // [4]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < p.C; c += ES_THREADS) seen[c] = 0;
    for (int j = tid; j < p.M; j += ES_THREADS) {
        const long long c1 = p.gt_cls[(long long)b * p.M + j];
        gcls[j] = (c1 >= 1 && c1 <= p.C) ? (int)(c1 - 1) : -1;
        gdif[j] = (p.gt_difficult && p.gt_difficult[(long long)b * p.M + j]) ? 1 : 0;
        taken[j] = 0;
    }
    __syncthreads();
    // ground truth: instances that are not difficult; images in which the class occurs at all (object_detection_evaluation.py:132-139)
    for (int j = tid; j < p.M; j += ES_THREADS) {
        const int c = gcls[j];
        if (c < 0) continue;
        if (!gdif[j]) atomicAdd(p.gt_count + c, 1);
        bool first = true;
        for (int q = 0; q < j; ++q) first = first && gcls[q] != c;
        if (first) atomicAdd(p.gt_imgs + c, 1);
    }
    const int n = min(p.det_count[b], p.max_det);
    int kept = 0, nans = 0;                          // thread 0's
    for (int i = 0; i < p.max_det; ++i) {
        unsigned* out = p.flags + (long long)b * p.max_det + i;
        if (i >= n) { if (tid == 0) *out = ES_INVALID; continue; }
        const float* d = p.det + ((long long)b * p.max_det + i) * 6;
        const float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3], score = d[4];
        const int c = (int)d[5] - 1;
        if (score != score) ++nans;
        if (!(y1 < y2 && x1 < x2) || c < 0 || c >= p.C || score != score) { if (tid == 0) *out = ES_INVALID; continue; }     // uniform
        const float area_d = (y2 - y1) * (x2 - x1);
        float best = -1.f; int bj = 0x7fffffff;
        for (int j = tid; j < p.M; j += ES_THREADS) {
            if (gcls[j] != c) continue;
            const float* g = p.gt_boxes + ((long long)b * p.M + j) * 4;             // yxyx
            const float ih = fmaxf(0.f, fminf(y2, g[2]) - fmaxf(y1, g[0]));
            const float iw = fmaxf(0.f, fminf(x2, g[3]) - fmaxf(x1, g[1]));
            const float inter = ih * iw;
            const float area_g = (g[2] - g[0]) * (g[3] - g[1]);
            const float iou = inter / (area_d + area_g - inter);
            if (iou > best) { best = iou; bj = j; }                                 // ascending j: first maximum kept
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
        if (tid == 0) {
            for (int w = 1; w < ES_WAVES; ++w)
                if (red_v[w] > best || (red_v[w] == best && red_i[w] < bj)) { best = red_v[w]; bj = red_i[w]; }
            const bool has_gt = bj != 0x7fffffff;
            unsigned word = 0, reach = 0;            // reach: thresholds the candidate's IoU reaches
            if (has_gt) {
                for (int t = 0; t < p.T; ++t) reach |= (best >= p.thr[t] ? 1u : 0u) << t;
                if (gdif[bj]) {
                    word = reach << 16;
                } else {
                    word = reach & ~(unsigned)taken[bj];
                    taken[bj] |= (int)reach;
                }
            }
            *out = word;
            if (!(word & ES_INVALID)) ++kept;             // T = 16: ignored at all 16 thresholds = bit 31 = dropped, the same thing
            if (!seen[c]) {                                                          // top-scoring detection of class c
                seen[c] = 1;
                for (int t = 0; t < p.T; ++t)
                    if ((reach >> t) & 1u) atomicAdd(p.correct + (long long)t * p.C + c, 1);
            }
        }
        __syncthreads();
    }
    if (tid == 0 && p.kept) { p.kept[b] = kept; p.kept[p.B + b] = nans; }
}

// ---- append ----------------------------------------------------------------------------------------------------------------------
struct EsAppend {
    const float* det; const unsigned* flags; const int* kept; int B, max_det;
    float* scores; int* classes; unsigned* out_flags; unsigned capacity; unsigned* state;     // state: {cursor, lost, NaN scores, 0}
    const unsigned* open; unsigned* out_open;                                                 // the open words (null: none), same positions
};

// workgroup b: image b's valid slots, in slot order, from cursor + the kept counts of the images before it
__global__ __launch_bounds__(ES_THREADS) void es_append_write_kernel(EsAppend a) {
    __shared__ unsigned shu[ES_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned before = 0;
    for (int k = tid; k < b; k += ES_THREADS) before += (unsigned)a.kept[k];
    unsigned pos = es_min(a.state[0], a.capacity) + es_block_sum<unsigned>(before, shu, tid);
    for (int i0 = 0; i0 < a.max_det; i0 += ES_THREADS) {
        const int i = i0 + tid;
        const long long slot = (long long)b * a.max_det + i;
        const unsigned f = i < a.max_det ? a.flags[slot] : ES_INVALID;
        const bool keep = !(f & ES_INVALID);
        unsigned total;
        const unsigned p = pos + es_block_excl_scan(keep ? 1u : 0u, shu, tid, &total);
        if (keep && p < a.capacity) {                                     // beyond the capacity: counted by the cursor launch
            float v = a.det[slot * 6 + 4];
            if (v == 0.f) v = 0.f;                                        // -0.0 is stored as +0.0: the two tie
            a.scores[p] = v;
            a.classes[p] = (int)a.det[slot * 6 + 5] - 1;
            a.out_flags[p] = f;
            if (a.out_open) a.out_open[p] = a.open[slot];
        }
        pos += total;
    }
}

// one workgroup: the cursor moves (clamped to the capacity; the surplus and the NaN scores are counted)
__global__ __launch_bounds__(ES_THREADS) void es_append_cursor_kernel(EsAppend a) {
    __shared__ unsigned shu[ES_WAVES];
    const int tid = threadIdx.x;
    unsigned kept = 0, nans = 0;
    for (int k = tid; k < a.B; k += ES_THREADS) { kept += (unsigned)a.kept[k]; nans += (unsigned)a.kept[a.B + k]; }
    kept = es_block_sum<unsigned>(kept, shu, tid);
    nans = es_block_sum<unsigned>(nans, shu, tid);
    if (tid == 0) {
        const u64 end = (u64)es_min(a.state[0], a.capacity) + kept;
        if (end > a.capacity) {
            const u64 lost = (u64)a.state[1] + (end - a.capacity);
            a.state[1] = lost > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)lost;
        }
        a.state[0] = end > a.capacity ? a.capacity : (unsigned)end;
        const u64 nn = (u64)a.state[2] + nans;
        a.state[2] = nn > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)nn;
    }
}

// ---- sort ------------------------------------------------------------------------------------------------------------------------
struct EsSort {
    const float* scores; const int* classes; const unsigned* flags;      // the first pass reads these
    const u64* src_k; const unsigned* src_v; u64* dst_k; unsigned* dst_v;
    const unsigned* open; const unsigned* src_w; unsigned* dst_w;         // a second payload word (the W2 scatter only)
    const unsigned* cursor; long long n_host;                             // live count: n_host, or min(*cursor, capacity) when n_host < 0
    unsigned* hist; unsigned* totals;
    unsigned capacity, tiles;                                             // tiles by capacity: the row pitch of hist
    int shift, first, C;
};

DEV unsigned es_live(const unsigned* cursor, long long n_host, unsigned capacity) {
    return n_host >= 0 ? (unsigned)n_host : es_min(cursor[0], capacity);
}
// (class << 32) | ~key(score): ascending = class, then score descending.  Invalid entries (flag bit 31, class outside 0..C-1, NaN
// score) get class C: behind every class.
DEV void es_sort_load(const EsSort& s, unsigned i, u64* key, unsigned* val) {
    if (!s.first) { *key = s.src_k[i]; *val = s.src_v[i]; return; }
    const unsigned f = s.flags[i];
    const int c = s.classes[i];
    float v = s.scores[i];
    const bool ok = !(f & ES_INVALID) && c >= 0 && c < s.C && v == v;
    if (v == 0.f) v = 0.f;
    *key = ((u64)(ok ? (unsigned)c : (unsigned)s.C) << 32) | (u64)(~es_key(__float_as_uint(v)));
    *val = f;
}

__global__ __launch_bounds__(ES_THREADS) void es_sort_hist_kernel(EsSort s) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    const unsigned n = es_live(s.cursor, s.n_host, s.capacity), tile = blockIdx.x;
    if (tile >= (n + ES_SORT_TILE - 1) / ES_SORT_TILE) return;          // the same for the whole workgroup
    h[tid] = 0;
    __syncthreads();
    for (int r = 0; r < ES_SORT_ITEMS; ++r) {
        const unsigned i = tile * ES_SORT_TILE + r * ES_THREADS + tid;
        if (i < n) {
            u64 k; unsigned v;
            es_sort_load(s, i, &k, &v);
            atomicAdd(&h[(unsigned)(k >> s.shift) & 255u], 1u);          // integer counts in LDS: order independent
        }
    }
    __syncthreads();
    s.hist[(unsigned)tid * s.tiles + tile] = h[tid];
}

// workgroup d: exclusive prefix of digit d's counts over the live tiles (in place), and the digit's total
__global__ __launch_bounds__(ES_THREADS) void es_sort_scan_kernel(EsSort s) {
    __shared__ unsigned sh[ES_WAVES];
    const int tid = threadIdx.x;
    const unsigned n = es_live(s.cursor, s.n_host, s.capacity), ntiles = (n + ES_SORT_TILE - 1) / ES_SORT_TILE;
    unsigned* row = s.hist + (unsigned)blockIdx.x * s.tiles;
    const unsigned chunk = (ntiles + ES_THREADS - 1) / ES_THREADS;
    const unsigned lo = es_min((unsigned)tid * chunk, ntiles), hi = es_min(lo + chunk, ntiles);
    unsigned sum = 0;
    for (unsigned k = lo; k < hi; ++k) sum += row[k];
    unsigned total;
    unsigned run = es_block_excl_scan(sum, sh, tid, &total);
    for (unsigned k = lo; k < hi; ++k) { const unsigned c = row[k]; row[k] = run; run += c; }
    if (tid == 0) s.totals[blockIdx.x] = total;
}

// Stable scatter of one tile.  Wave w owns entries [w * 1024, (w + 1) * 1024) of the tile, 64 consecutive ones per round.  An entry's
// rank among the equal digits of its wave = the wave's running count of the digit + the equal digits in lower lanes (ballots); the
// waves' counts are then prefixed per digit on top of (digits below in the array) + (this digit in earlier tiles).
template <bool W2> __global__ __launch_bounds__(ES_THREADS) void es_sort_scatter_kernel(EsSort s) {
    __shared__ unsigned wcnt[ES_WAVES][256];
    __shared__ unsigned sh[ES_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned n = es_live(s.cursor, s.n_host, s.capacity), tile = blockIdx.x;
    if (tile >= (n + ES_SORT_TILE - 1) / ES_SORT_TILE) return;
    for (int w = 0; w < ES_WAVES; ++w) wcnt[w][tid] = 0;
    unsigned total;
    const unsigned digit_first = es_block_excl_scan(s.totals[tid], sh, tid, &total) + s.hist[(unsigned)tid * s.tiles + tile];
    // (the scan's barriers also publish the zeroed counters)
    const u64 below = (1ull << lane) - 1ull;
    const unsigned seg = tile * ES_SORT_TILE + (unsigned)wave * (64 * ES_SORT_ITEMS);
    u64 key[ES_SORT_ITEMS];
    unsigned val[ES_SORT_ITEMS], rank[ES_SORT_ITEMS], val2[W2 ? ES_SORT_ITEMS : 1];
#pragma unroll
    for (int r = 0; r < ES_SORT_ITEMS; ++r) {
        const unsigned i = seg + r * 64 + lane;
        const bool valid = i < n;
        u64 k = ~0ull; unsigned v = 0;
        if (valid) es_sort_load(s, i, &k, &v);
        if constexpr (W2) val2[r] = valid ? (s.first ? s.open[i] : s.src_w[i]) : 0u;
        const unsigned d = (unsigned)(k >> s.shift) & 255u;
        u64 same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const u64 bal = __ballot(on);
            same &= on ? bal : ~bal;
        }
        const unsigned lower = es_popc(same & below);
        const unsigned prev = valid ? wcnt[wave][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && lower == 0) wcnt[wave][d] = prev + es_popc(same);     // one lane per digit present in the round
        __builtin_amdgcn_wave_barrier();
        key[r] = k; val[r] = v;
        rank[r] = prev + lower;
    }
    __syncthreads();
    {   // thread d: the waves' counts of digit d -> first positions
        unsigned run = digit_first;
        for (int w = 0; w < ES_WAVES; ++w) { const unsigned c = wcnt[w][tid]; wcnt[w][tid] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ES_SORT_ITEMS; ++r) {
        const unsigned i = seg + r * 64 + lane;
        if (i < n) {
            const unsigned p = wcnt[wave][(unsigned)(key[r] >> s.shift) & 255u] + rank[r];
            if (p < n) {
                s.dst_k[p] = key[r]; s.dst_v[p] = val[r];
                if constexpr (W2) s.dst_w[p] = val2[r];
            }
        }
    }
}

// ---- average precision -----------------------------------------------------------------------------------------------------------
struct EsAp {
    const u64* keys; const unsigned* flags;                               // sorted
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C;
    const int* gt_count; const int* gt_imgs; const int* correct;
    u64* result;
};

// workgroup (c, t): AP of class c at threshold t, and the (c, t) entries of the result block
__global__ __launch_bounds__(ES_THREADS) void es_ap_kernel(EsAp a) {
    __shared__ unsigned shu[ES_WAVES];
    __shared__ double shd[ES_WAVES];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const unsigned n = es_live(a.state, a.n_host, a.capacity);
    const unsigned s = es_lower_bound(a.keys, n, (u64)c << 32), e = es_lower_bound(a.keys, n, (u64)(c + 1) << 32);
    const int ng = a.gt_count[c];
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    double acc = 0.0;
    if (ng > 0 && e > s) {                                                // the same for the whole workgroup
        unsigned tot = 0;                                                 // not ignored | true positives << 16 per thread: < 2^16 each
        unsigned rem_ni = 0, rem_tp = 0;
        for (unsigned i0 = s; i0 < e; i0 += ES_THREADS * 256) {           // a thread adds up to 256 entries before the sums are unpacked
            tot = 0;
            unsigned i = i0 + tid;
            for (unsigned r = 0; r < 256 && i < e; ++r, i += ES_THREADS) {
                const unsigned f = a.flags[i];
                tot += ((f & ig_bit) ? 0u : 1u) + ((f & tp_bit) ? 0x10000u : 0u);
            }
            rem_ni += es_block_sum<unsigned>(tot & 0xFFFFu, shu, tid);
            rem_tp += es_block_sum<unsigned>(tot >> 16, shu, tid);
        }
        const double dng = (double)ng;
        double carry = 0.0;                                               // largest precision of the chunks behind this one
        const unsigned nchunks = (e - s + ES_AP_CHUNK - 1) / ES_AP_CHUNK;
        for (unsigned q = nchunks; q-- > 0;) {
            const unsigned i0 = s + q * ES_AP_CHUNK + (unsigned)tid * ES_AP_ITEMS;
            unsigned f[ES_AP_ITEMS], cnt = 0;
#pragma unroll
            for (int r = 0; r < ES_AP_ITEMS; ++r) {
                f[r] = i0 + r < e ? a.flags[i0 + r] : ig_bit;              // beyond the segment: ignored
                cnt += ((f[r] & ig_bit) ? 0u : 1u) + ((f[r] & tp_bit) ? 0x10000u : 0u);
            }
            unsigned total;
            const unsigned ex = es_block_excl_scan(cnt, shu, tid, &total);
            rem_ni -= total & 0xFFFFu; rem_tp -= total >> 16;             // now: the counts in front of this chunk
            unsigned rank = rem_ni + (ex & 0xFFFFu), ctp = rem_tp + (ex >> 16);
            double prec[ES_AP_ITEMS], step[ES_AP_ITEMS];
#pragma unroll
            for (int r = 0; r < ES_AP_ITEMS; ++r) {
                const bool ni = !(f[r] & ig_bit), tp = f[r] & tp_bit;
                rank += ni ? 1u : 0u; ctp += tp ? 1u : 0u;
                prec[r] = ni ? (double)ctp / (double)rank : 0.0;
                step[r] = tp ? (double)ctp / dng - (double)(ctp - 1u) / dng : 0.0;
            }
#pragma unroll
            for (int r = ES_AP_ITEMS - 2; r >= 0; --r) prec[r] = fmax(prec[r], prec[r + 1]);      // envelope inside the thread
            double chunk_max;
            const double later = fmax(es_block_excl_rmax(prec[0], shd, tid, &chunk_max), carry);
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < ES_AP_ITEMS; ++r)
                if (f[r] & tp_bit) sum += step[r] * fmax(prec[r], later);
            acc += es_block_sum<double>(sum, shd, tid);
            carry = fmax(carry, chunk_max);
        }
    }
    if (tid != 0) return;
    u64* res = a.result;
    double* ap = reinterpret_cast<double*>(res + ES_RESULT_HEAD);
    long long* cnt = reinterpret_cast<long long*>(res + ES_RESULT_HEAD + (long long)a.T * a.C);
    ap[(long long)t * a.C + c] = ng > 0 ? acc : __builtin_nan("");
    cnt[2ll * a.C + (long long)t * a.C + c] = a.correct[(long long)t * a.C + c];
    if (t == 0) { cnt[c] = ng; cnt[a.C + c] = a.gt_imgs[c]; }
    if (t == 0 && c == 0) {
        res[0] = n; res[1] = a.state ? a.state[1] : 0; res[2] = a.state ? a.state[2] : 0; res[3] = (u64)a.T; res[4] = (u64)a.C;
        res[5] = 0; res[6] = 0; res[7] = 0;
    }
}

// ---- open-set protocol: known classes 0 .. C-2, the unknown class U = C-1 (0-based) -------------------------------------------------
constexpr int ES_OPEN_CHUNK = ES_THREADS;                             // unknown boxes staged in LDS at a time
constexpr int ES_OPEN_MATS = 7;                                       // n_det, tp, open_total, k_star, pos, rank_at, open_at

struct EsOpenWords {
    const float* det; const unsigned* flags; const float* gt_boxes; const long long* gt_cls;
    int B, max_det, M, U, T; float thr[ES_MAX_T];                     // U: the 1-based unknown class
    unsigned* open;
};

// workgroup b: bit t of a kept known-class detection = its largest IoU with the image's boxes of class U reaches thr[t].  No greedy
// state: a detection per thread; the unknown boxes pass through LDS ES_OPEN_CHUNK ground-truth rows at a time, compacted, so every
// thread reads the same LDS word (a broadcast).  A maximum over `>` does not depend on the order of the boxes.
__global__ __launch_bounds__(ES_THREADS) void es_open_words_kernel(EsOpenWords p) {
    __shared__ float box[ES_OPEN_CHUNK][4];
    __shared__ unsigned shu[ES_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int i0 = 0; i0 < p.max_det; i0 += ES_THREADS) {
        const int i = i0 + tid;
        const long long slot = (long long)b * p.max_det + i;
        bool live = false;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
        if (i < p.max_det) {
            const float* d = p.det + slot * 6;
            const int c1 = (int)d[5];
            live = !(p.flags[slot] & ES_INVALID) && c1 >= 1 && c1 < p.U;
            x1 = d[0]; y1 = d[1]; x2 = d[2]; y2 = d[3];
        }
        const float area_d = (y2 - y1) * (x2 - x1);
        float best = -__builtin_inff();
        for (int j0 = 0; j0 < p.M; j0 += ES_OPEN_CHUNK) {             // uniform trip count
            const int j = j0 + tid;
            const bool unk = j < p.M && p.gt_cls[(long long)b * p.M + j] == (long long)p.U;
            unsigned cnt;
            const unsigned at = es_block_excl_scan(unk ? 1u : 0u, shu, tid, &cnt);      // at < ES_OPEN_CHUNK
            if (unk) {
                const float* g = p.gt_boxes + ((long long)b * p.M + j) * 4;
                box[at][0] = g[0]; box[at][1] = g[1]; box[at][2] = g[2]; box[at][3] = g[3];
            }
            __syncthreads();
            if (live)
                for (unsigned k = 0; k < cnt; ++k) {
                    const float g0 = box[k][0], g1 = box[k][1], g2 = box[k][2], g3 = box[k][3];      // yxyx
                    const float ih = fmaxf(0.f, fminf(y2, g2) - fmaxf(y1, g0));
                    const float iw = fmaxf(0.f, fminf(x2, g3) - fmaxf(x1, g1));
                    const float inter = ih * iw;
                    const float area_g = (g2 - g0) * (g3 - g1);
                    const float iou = inter / (area_d + area_g - inter);
                    if (iou > best) best = iou;
                }
            __syncthreads();                                          // the chunk is free again
        }
        if (i < p.max_det) {
            unsigned word = 0;
            if (live)
                for (int t = 0; t < p.T; ++t) word |= (best >= p.thr[t] ? 1u : 0u) << t;
            p.open[slot] = word;
        }
    }
}

struct EsOpenCounts {
    const u64* keys; const unsigned* flags; const unsigned* open;        // sorted
    const unsigned* state; long long n_host; unsigned capacity;
    int T, C; double level;
    const int* gt_count;
    long long* mats;                                                      // [ES_OPEN_MATS][T][C]
};

// entries [s, e) of one segment: not ignored at t, true positives at t, open bit t (three sums in a fixed order)
DEV void es_open_totals(const EsOpenCounts& a, unsigned s, unsigned e, unsigned tp_bit, unsigned ig_bit, unsigned* shu, int tid,
                        unsigned* ni, unsigned* tp, unsigned* op) {
    unsigned c_ni = 0, c_tp = 0, c_op = 0;                                // a thread sees at most 2^24 / 256 entries
    for (unsigned i = s + tid; i < e; i += ES_THREADS) {
        const unsigned f = a.flags[i];
        c_ni += (f & ig_bit) ? 0u : 1u; c_tp += (f & tp_bit) ? 1u : 0u; c_op += (a.open[i] & tp_bit) ? 1u : 0u;
    }
    *ni = es_block_sum<unsigned>(c_ni, shu, tid);
    *tp = es_block_sum<unsigned>(c_tp, shu, tid);
    *op = es_block_sum<unsigned>(c_op, shu, tid);
}

// workgroup (c, t): the counts of class c at threshold t.  Pass 1: the totals, then k_star = the reachable cumulative-TP count
// whose recall is nearest the level (float64, ties to the smaller count; the candidates floor(level n_gt) - 1 .. + 2 suffice).
// Pass 2: the first position with that count (the chunks from the front, an integer scan each), and the counts up to it.
__global__ __launch_bounds__(ES_THREADS) void es_open_counts_kernel(EsOpenCounts a) {
    __shared__ unsigned shu[ES_WAVES];
    __shared__ unsigned sh_pos;
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const unsigned n = es_live(a.state, a.n_host, a.capacity);
    const unsigned s = es_lower_bound(a.keys, n, (u64)c << 32), e = es_lower_bound(a.keys, n, (u64)(c + 1) << 32);
    const int ng = a.gt_count[c];
    const unsigned tp_bit = 1u << t, ig_bit = 1u << (16 + t);
    unsigned n_det, tp, open_total;
    es_open_totals(a, s, e, tp_bit, ig_bit, shu, tid, &n_det, &tp, &open_total);
    long long k_star = 0, pos = -1, rank_at = 0, open_at = 0;
    if (ng > 0 && e > s) {                                                // the same for the whole workgroup
        const long long k_min = (a.flags[s] & tp_bit) ? 1 : 0, k_max = (long long)tp;
        const double dng = (double)ng;
        const long long base = (long long)floor(a.level * dng);
        double best = 0.0;
        bool have = false;
        for (long long d = -1; d <= 2; ++d) {
            long long k = base + d;
            k = k < k_min ? k_min : (k > k_max ? k_max : k);              // ascending in d: the first minimum is the smaller count
            const double dist = fabs((double)k / dng - a.level);
            if (!have || dist < best) { best = dist; k_star = k; have = true; }
        }
        unsigned first = s;                                               // k_star = 0: position 0 (k_min is 0 then)
        if (k_star > 0) {
            const unsigned want = (unsigned)k_star;
            unsigned seen = 0;
            bool found = false;
            const unsigned nchunks = (e - s + ES_AP_CHUNK - 1) / ES_AP_CHUNK;
            for (unsigned q = 0; q < nchunks && !found; ++q) {            // `found` is the same for the whole workgroup
                const unsigned i0 = s + q * ES_AP_CHUNK + (unsigned)tid * ES_AP_ITEMS;
                unsigned f[ES_AP_ITEMS], cnt = 0;
#pragma unroll
                for (int r = 0; r < ES_AP_ITEMS; ++r) {
                    f[r] = i0 + r < e ? a.flags[i0 + r] : 0u;
                    cnt += (f[r] & tp_bit) ? 1u : 0u;
                }
                unsigned total;
                unsigned run = seen + es_block_excl_scan(cnt, shu, tid, &total);
                if (run < want && want <= run + cnt) {                    // one thread of one chunk
#pragma unroll
                    for (int r = 0; r < ES_AP_ITEMS; ++r) {
                        if (f[r] & tp_bit) { ++run; if (run == want) sh_pos = i0 + r; }
                    }
                }
                __syncthreads();
                found = seen + total >= want;
                if (found) first = sh_pos;
                seen += total;
            }
        }
        pos = (long long)(first - s);
        unsigned ni_at, tp_at, op_at;
        es_open_totals(a, s, first + 1, tp_bit, ig_bit, shu, tid, &ni_at, &tp_at, &op_at);
        rank_at = ni_at; open_at = op_at;
    }
    if (tid != 0) return;
    const long long TC = (long long)a.T * a.C, at = (long long)t * a.C + c;
    a.mats[0 * TC + at] = n_det; a.mats[1 * TC + at] = tp; a.mats[2 * TC + at] = open_total;
    a.mats[3 * TC + at] = k_star; a.mats[4 * TC + at] = pos; a.mats[5 * TC + at] = rank_at; a.mats[6 * TC + at] = open_at;
}

// ---- relabelling below a score threshold --------------------------------------------------------------------------------------------
struct EsRelabel {
    const float* det_in; const int* count; const float* score; long long pitch, stride;
    int B, max_det, C; float tau; const float* tau_dev; float* det_out;
};

// thread (b, j): row j of image b, its class set to C + 1 where j < count[b], the class is in 1..C and !(score >= tau)
__global__ __launch_bounds__(ES_THREADS) void es_relabel_unknown_kernel(EsRelabel p) {
    const long long row = (long long)blockIdx.x * ES_THREADS + threadIdx.x;
    if (row >= (long long)p.B * p.max_det) return;
    const int b = (int)(row / p.max_det), j = (int)(row % p.max_det);
    const float tau = p.tau_dev ? p.tau_dev[0] : p.tau;
    const float* d = p.det_in + row * 6;
    const float v0 = d[0], v1 = d[1], v2 = d[2], v3 = d[3], v4 = d[4];
    float cls = d[5];
    const int c1 = (int)cls;
    if (j < p.count[b] && c1 >= 1 && c1 <= p.C && !(p.score[(long long)b * p.pitch + (long long)j * p.stride] >= tau))
        cls = (float)(p.C + 1);
    float* o = p.det_out + row * 6;
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; o[4] = v4; o[5] = cls;
}

// ---- workspace layout (host) -------------------------------------------------------------------------------------------------------
struct EsLayout { long long keys[2], vals[2], vals2[2], hist, totals, total; unsigned tiles; int passes; };

int es_append(void* stream, const EsAppend& a) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(es_append_write_kernel, dim3(a.B), dim3(ES_THREADS), 0, st, a);
    hipLaunchKernelGGL(es_append_cursor_kernel, dim3(1), dim3(ES_THREADS), 0, st, a);
    return effdet_check_launch();
}

bool es_layout(long long capacity, int C, EsLayout* L, bool open = false) {
    if (capacity < 1 || capacity > ES_MAX_N || C < 1 || C > ES_MAX_C) return false;
    long long off = 0;
    auto take = [&off](long long bytes) { const long long o = off; off += (bytes + 255) & ~255ll; return o; };
    L->tiles = (unsigned)((capacity + ES_SORT_TILE - 1) / ES_SORT_TILE);
    L->passes = C <= 255 ? 5 : 6;                                         // 4 score digits, then the class (C itself is a key)
    for (int k = 0; k < 2; ++k) { L->keys[k] = take(capacity * 8); L->vals[k] = take(capacity * 4); }
    for (int k = 0; k < 2; ++k) L->vals2[k] = open ? take(capacity * 4) : 0;
    L->hist = take(256ll * L->tiles * 4);
    L->totals = take(256 * 4);
    L->total = off;
    return true;
}

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------------
extern "C" int effdet_eval_scale_sort_tile(void) { return ES_SORT_TILE; }

extern "C" int effdet_eval_match_multi(void* stream, const float* det, const int* det_count, const float* gt_boxes,
                                       const long long* gt_cls, const unsigned char* gt_difficult, int B, int max_det, int M,
                                       int num_classes, const float* thresholds, int num_thresholds, unsigned int* flags, int* kept,
                                       int* gt_count, int* gt_imgs, int* correct_imgs) {
    EFFDET_ENTER();
    if (!det || !det_count || !gt_boxes || !gt_cls || !thresholds || !flags || !gt_count || !gt_imgs || !correct_imgs)
        return EFFDET_EINVAL;      // null pointer
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16
    for (int t = 0; t < num_thresholds; ++t)
        if (!(thresholds[t] == thresholds[t]) || (t > 0 && !(thresholds[t] > thresholds[t - 1])))
            return EFFDET_EINVAL;      // thresholds must ascend
    if (B <= 0 || max_det <= 0 || M <= 0 || (long long)B * max_det > ES_MAX_N) return EFFDET_EINVAL;      // bad B, max_det or M
    if (num_classes < 1 || num_classes > ES_MAX_C) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    const size_t sh = ((size_t)num_classes + 3 * (size_t)M + 8) * sizeof(int);
    if (sh > 64 * 1024) return EFFDET_EINVAL;      // (num_classes + 3 M + 8) ints exceed 64 KiB of LDS
    EsMatch a;
    a.det = det; a.det_count = det_count; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls; a.gt_difficult = gt_difficult;
    a.B = B; a.max_det = max_det; a.M = M; a.C = num_classes; a.T = num_thresholds;
    for (int t = 0; t < ES_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.flags = flags; a.kept = kept; a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    hipLaunchKernelGGL(es_match_kernel, dim3(B), dim3(ES_THREADS), sh, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_eval_append(void* stream, const float* det, const unsigned int* flags, const int* kept, int B, int max_det,
                                  float* scores, int* classes, unsigned int* out_flags, long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !kept || !scores || !classes || !out_flags || !state) return EFFDET_EINVAL;      // null pointer
    if (B <= 0 || max_det <= 0 || (long long)B * max_det > ES_MAX_N) return EFFDET_EINVAL;      // bad B or max_det
    if (capacity < 1 || capacity > ES_MAX_N) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    EsAppend a{det, flags, kept, B, max_det, scores, classes, out_flags, (unsigned)capacity, state, nullptr, nullptr};
    return es_append(stream, a);
}

extern "C" int effdet_eval_append_open(void* stream, const float* det, const unsigned int* flags, const unsigned int* open,
                                       const int* kept, int B, int max_det, float* scores, int* classes, unsigned int* out_flags,
                                       unsigned int* out_open, long long capacity, unsigned int* state) {
    EFFDET_ENTER();
    if (!det || !flags || !open || !kept || !scores || !classes || !out_flags || !out_open || !state)
        return EFFDET_EINVAL;      // null pointer
    if (B <= 0 || max_det <= 0 || (long long)B * max_det > ES_MAX_N) return EFFDET_EINVAL;      // bad B or max_det
    if (capacity < 1 || capacity > ES_MAX_N) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    EsAppend a{det, flags, kept, B, max_det, scores, classes, out_flags, (unsigned)capacity, state, open, out_open};
    return es_append(stream, a);
}

extern "C" long long effdet_eval_ap_sorted_workspace_bytes(long long capacity, int num_classes) {
    EsLayout L;
    return es_layout(capacity, num_classes, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_eval_ap_sorted_offset(long long capacity, int num_classes, int which) {
    EsLayout L;
    if ((which != 0 && which != 1) || !es_layout(capacity, num_classes, &L)) return EFFDET_EINVAL;
    const int last = (L.passes - 1) & 1;
    return which == 0 ? L.keys[last] : L.vals[last];
}

extern "C" long long effdet_eval_ap_sorted_result_bytes(int num_thresholds, int num_classes) {
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T || num_classes < 1 || num_classes > ES_MAX_C) return EFFDET_EINVAL;
    return 8ll * (ES_RESULT_HEAD + 2ll * num_thresholds * num_classes + 2ll * num_classes);
}

// sort + AP (+ the open-set counts when `open` is given): the body of effdet_eval_ap_sorted and effdet_eval_open_sorted
static int es_sorted_run(void* stream, const float* scores, const int* classes, const unsigned int* flags, const unsigned int* open,
                         long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes,
                         const int* gt_count, const int* gt_imgs, const int* correct_imgs, double level, void* workspace,
                         long long workspace_bytes, void* result) {
    if (!scores || !classes || !flags || !gt_count || !gt_imgs || !correct_imgs || !workspace || !result)
        return EFFDET_EINVAL;      // null pointer
    if (n < 0 && !state) return EFFDET_EINVAL;      // n < 0 takes the count from `state`, which is null
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16
    if (num_classes < 1 || num_classes > ES_MAX_C) return EFFDET_EINVAL;      // 1 <= num_classes <= 65535
    EsLayout L;
    if (!es_layout(capacity, num_classes, &L, open != nullptr)) return EFFDET_EINVAL;      // 1 <= capacity <= 2^24
    if (n > capacity) return EFFDET_EINVAL;      // n exceeds the capacity
    if (workspace_bytes < L.total) return EFFDET_EINVAL;      // workspace too small
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(result) % 8)
        return EFFDET_EINVAL;      // workspace and result must be 8-byte aligned
    char* ws = reinterpret_cast<char*>(workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    EsSort s;
    s.scores = scores; s.classes = classes; s.flags = flags; s.open = open;
    s.cursor = state; s.n_host = n < 0 ? -1 : n;
    s.hist = reinterpret_cast<unsigned*>(ws + L.hist); s.totals = reinterpret_cast<unsigned*>(ws + L.totals);
    s.capacity = (unsigned)capacity; s.tiles = L.tiles; s.C = num_classes;
    const unsigned grid = n < 0 ? L.tiles : (unsigned)((n + ES_SORT_TILE - 1) / ES_SORT_TILE);
    for (int pass = 0; pass < L.passes && grid > 0; ++pass) {
        const int d = pass & 1;                                           // in -> 0 -> 1 -> 0 ...
        s.shift = 8 * pass; s.first = pass == 0;
        s.src_k = reinterpret_cast<const u64*>(ws + L.keys[1 - d]); s.src_v = reinterpret_cast<const unsigned*>(ws + L.vals[1 - d]);
        s.dst_k = reinterpret_cast<u64*>(ws + L.keys[d]); s.dst_v = reinterpret_cast<unsigned*>(ws + L.vals[d]);
        s.src_w = open ? reinterpret_cast<const unsigned*>(ws + L.vals2[1 - d]) : nullptr;
        s.dst_w = open ? reinterpret_cast<unsigned*>(ws + L.vals2[d]) : nullptr;
        hipLaunchKernelGGL(es_sort_hist_kernel, dim3(grid), dim3(ES_THREADS), 0, st, s);
        hipLaunchKernelGGL(es_sort_scan_kernel, dim3(256), dim3(ES_THREADS), 0, st, s);
        if (open) hipLaunchKernelGGL(es_sort_scatter_kernel<true>, dim3(grid), dim3(ES_THREADS), 0, st, s);
        else hipLaunchKernelGGL(es_sort_scatter_kernel<false>, dim3(grid), dim3(ES_THREADS), 0, st, s);
    }
    const int last = (L.passes - 1) & 1;
    EsAp a;
    a.keys = reinterpret_cast<const u64*>(ws + L.keys[last]); a.flags = reinterpret_cast<const unsigned*>(ws + L.vals[last]);
    a.state = state; a.n_host = s.n_host; a.capacity = (unsigned)capacity;
    a.T = num_thresholds; a.C = num_classes;
    a.gt_count = gt_count; a.gt_imgs = gt_imgs; a.correct = correct_imgs;
    a.result = reinterpret_cast<u64*>(result);
    hipLaunchKernelGGL(es_ap_kernel, dim3((unsigned)num_classes, (unsigned)num_thresholds), dim3(ES_THREADS), 0, st, a);
    if (open) {
        EsOpenCounts o;
        o.keys = a.keys; o.flags = a.flags; o.open = reinterpret_cast<const unsigned*>(ws + L.vals2[last]);
        o.state = state; o.n_host = s.n_host; o.capacity = (unsigned)capacity;
        o.T = num_thresholds; o.C = num_classes; o.level = level;
        o.gt_count = gt_count;
        o.mats = reinterpret_cast<long long*>(result) + ES_RESULT_HEAD + 2ll * num_thresholds * num_classes + 2ll * num_classes;
        hipLaunchKernelGGL(es_open_counts_kernel, dim3((unsigned)num_classes, (unsigned)num_thresholds), dim3(ES_THREADS), 0, st, o);
    }
    return effdet_check_launch();
}

extern "C" int effdet_eval_ap_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                     long long capacity, long long n, const unsigned int* state, int num_thresholds, int num_classes,
                                     const int* gt_count, const int* gt_imgs, const int* correct_imgs, void* workspace,
                                     long long workspace_bytes, void* result) {
    EFFDET_ENTER();
    return es_sorted_run(stream, scores, classes, flags, nullptr, capacity, n, state, num_thresholds, num_classes, gt_count, gt_imgs,
                         correct_imgs, 0.0, workspace, workspace_bytes, result);
}

// ---- open-set protocol: C ABI (num_classes counts the unknown class: known classes 1 .. num_classes - 1) -----------------------------
extern "C" int effdet_eval_open_words(void* stream, const float* det, const unsigned int* flags, const float* gt_boxes,
                                      const long long* gt_cls, int B, int max_det, int M, int num_classes, const float* thresholds,
                                      int num_thresholds, unsigned int* open) {
    EFFDET_ENTER();
    if (!det || !flags || !gt_boxes || !gt_cls || !thresholds || !open) return EFFDET_EINVAL;      // null pointer
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T) return EFFDET_EINVAL;      // 1 <= num_thresholds <= 16
    for (int t = 0; t < num_thresholds; ++t)
        if (!(thresholds[t] == thresholds[t]) || (t > 0 && !(thresholds[t] > thresholds[t - 1])))
            return EFFDET_EINVAL;      // thresholds must ascend
    if (B <= 0 || max_det <= 0 || M <= 0 || (long long)B * max_det > ES_MAX_N) return EFFDET_EINVAL;      // bad B, max_det or M
    if (num_classes < 2 || num_classes > ES_MAX_C) return EFFDET_EINVAL;      // 2 <= num_classes <= 65535
    EsOpenWords a;
    a.det = det; a.flags = flags; a.gt_boxes = gt_boxes; a.gt_cls = gt_cls;
    a.B = B; a.max_det = max_det; a.M = M; a.U = num_classes; a.T = num_thresholds;
    for (int t = 0; t < ES_MAX_T; ++t) a.thr[t] = t < num_thresholds ? thresholds[t] : 0.f;
    a.open = open;
    hipLaunchKernelGGL(es_open_words_kernel, dim3(B), dim3(ES_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" long long effdet_eval_open_sorted_workspace_bytes(long long capacity, int num_classes) {
    EsLayout L;
    return es_layout(capacity, num_classes, &L, true) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" long long effdet_eval_open_sorted_offset(long long capacity, int num_classes, int which) {
    EsLayout L;
    if (which < 0 || which > 2 || !es_layout(capacity, num_classes, &L, true)) return EFFDET_EINVAL;
    const int last = (L.passes - 1) & 1;
    return which == 0 ? L.keys[last] : which == 1 ? L.vals[last] : L.vals2[last];
}

extern "C" long long effdet_eval_open_sorted_result_bytes(int num_thresholds, int num_classes) {
    if (num_thresholds < 1 || num_thresholds > ES_MAX_T || num_classes < 2 || num_classes > ES_MAX_C) return EFFDET_EINVAL;
    return 8ll * (ES_RESULT_HEAD + (2ll + ES_OPEN_MATS) * num_thresholds * num_classes + 2ll * num_classes);
}

extern "C" int effdet_eval_open_sorted(void* stream, const float* scores, const int* classes, const unsigned int* flags,
                                       const unsigned int* open, long long capacity, long long n, const unsigned int* state,
                                       int num_thresholds, int num_classes, const int* gt_count, const int* gt_imgs,
                                       const int* correct_imgs, double recall_level, void* workspace, long long workspace_bytes,
                                       void* result) {
    EFFDET_ENTER();
    if (!open) return EFFDET_EINVAL;      // null pointer
    if (num_classes < 2) return EFFDET_EINVAL;      // 2 <= num_classes <= 65535
    if (!(recall_level > 0.0 && recall_level <= 1.0)) return EFFDET_EINVAL;      // recall_level must lie in (0, 1]
    return es_sorted_run(stream, scores, classes, flags, open, capacity, n, state, num_thresholds, num_classes, gt_count, gt_imgs,
                         correct_imgs, recall_level, workspace, workspace_bytes, result);
}

extern "C" int effdet_relabel_unknown(void* stream, const float* det_in, const int* count, const float* score, long long pitch,
                                      long long stride, int B, int max_det, int num_known, float tau, const float* tau_device,
                                      float* det_out) {
    EFFDET_ENTER();
    if (!det_in || !count || !score || !det_out) return EFFDET_EINVAL;      // null pointer
    if (B <= 0 || max_det <= 0 || (long long)B * max_det > ES_MAX_N) return EFFDET_EINVAL;      // bad B or max_det
    if (num_known < 1 || num_known >= ES_MAX_C) return EFFDET_EINVAL;      // 1 <= num_known <= 65534
    if (pitch < 0 || stride < 0) return EFFDET_EINVAL;      // negative pitch or stride
    EsRelabel a{det_in, count, score, pitch, stride, B, max_det, num_known, tau, tau_device, det_out};
    const unsigned grid = (unsigned)(((long long)B * max_det + ES_THREADS - 1) / ES_THREADS);
    hipLaunchKernelGGL(es_relabel_unknown_kernel, dim3(grid), dim3(ES_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}
