// Nearest-neighbour feature OOD score on the device: a bank of in-distribution pyramid rows and the squared distance of
// a query row to its k-th nearest bank row ("deep nearest neighbours", Sun et al. 2022), with the nearest row and its class.
//
//   append  the valid rows of a [B, K] call -> the bank at a device cursor, in (b, j) order: the ordered compaction of compact.h
//           (its base launch also moves the counters) gives every entry its bank row, then the rows themselves, four lanes a row.
//           The valid
//           row with global ordinal g (counted since the last clear, across calls) is kept when g % sample_every == 0 and lands on
//           row size0 + g / s - ceil(seen0 / s): the bank does not depend on how the rows are split into calls.
//   score   launch 1, grid (64-row block, bank split): a wave holds its 16 normalised query rows as the B operand in registers
//           (F / 4 values a lane), the workgroup walks its split of the bank 32 rows (16 at F = 288) a step through double-buffered
//           LDS as the A operand of v_mfma_f32_16x16x4_f32, so the four accumulator values of a lane belong to one query: each
//           lane keeps an ascending list of the KL smallest d2 it has seen (a compare-exchange chain behind a wave ballot) and
//           its own nearest (d2, i).  launch 2, a wave per row: the 4 x splits lists -> the k-th smallest value, the
//           lexicographic minimum of (d2, i) and the class.
//
// d2_i = max((|q|^2 + |r_i|^2) - 2 q.r_i, 0) is one fixed float32 expression per (query, bank row) pair - the dot product is the
// MFMA's fmaf chain over k in a fixed order - and the selection is a function of the multiset, so the outputs are bit-identical
// for every split count.  |x|^2 is summed in one fixed order everywhere (fk_tree4x4): 16 partial sums over k mod 16, then a tree.
// Every row index is compared with its table before a pointer is formed, every store index with its extent before the store; no
// call synchronises with the host or allocates, so all of them can be captured in a graph.
#include "common.h"
#include "feature_rows.h"

namespace {

constexpr int FK_MAX_K = 32;
constexpr int FK_MAX_SPLITS = 64;
constexpr int FK_CUS = 256;
constexpr long long FK_MAX_CAPACITY = 1ll << 24;
constexpr int FK_QROWS = 64;                                    // query rows of a workgroup, 16 per wave

DEV float fk_inf() { return __builtin_inff(); }

// |x|^2 of a row: 16 partial sums p[j] over k mod 16 == j (k ascending), then the tree (p[j] + p[j + 8]), (.. + 4), (.. + 2),
// (.. + 1) - here with the partial sums spread over the four lanes l, l ^ 16, l ^ 32, l ^ 48: lane group g holds p[4 g + s]
DEV float fk_tree4x4(const float (&p)[4]) {
    float t[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = p[s] + __shfl_xor(p[s], 32, 64);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = t[s] + __shfl_xor(t[s], 16, 64);
    return (t[0] + t[2]) + (t[1] + t[3]);
}
DEV float fk_inv_norm(float n2) { return 1.0f / sqrtf(fmaxf(n2, 1e-24f)); }

// ---- append ------------------------------------------------------------------------------------------------------------------
struct FkAppend {
    FoLevels L;
    FoSel sel;
    FoClasses cls;                                              // C = 0: no classes
    int F, Fp, A;
    int normalize;
    long long every, cap;
    float* bank; float* norms; int* bcls;                       // [cap][Fp], [cap], [cap]
    long long* counters;                                        // size, seen, lost
    long long* header;                                          // workspace: seen and size before this call
    unsigned* counts; unsigned nblocks;
    int* slots;                                                 // workspace: [total], the bank row of every entry or -1
};

// is entry i = b * K + j a valid row?
DEV bool fk_keep(const FkAppend& a, unsigned i, const char** row, int* cls) {
    unsigned b; long long an;
    if (!fo_select(a.sel, i, &b, &an)) return false;
    int cl = -1;
    if (a.cls.C > 0 && (cl = fo_class(a.cls, b, i - b * a.sel.K)) < 0) return false;
    *row = fo_row(a.L, b, (unsigned)(an / a.A));
    *cls = cl;
    return true;
}

DEV long long fk_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

DEV bool cp_keep(const FkAppend& a, unsigned i) { const char* row; int cl; return fk_keep(a, i, &row, &cl); }
DEV unsigned cp_begin(const FkAppend&) { return 0u; }
// the counters move on, their old values stay in the header
DEV void cp_finish(const FkAppend& a, unsigned, unsigned total) {
    const long long size0 = a.counters[0], seen0 = a.counters[1];
    a.header[0] = seen0; a.header[1] = size0;
    const long long kept = fk_ceil_div(seen0 + total, a.every) - fk_ceil_div(seen0, a.every);
    const long long room = a.cap > size0 ? a.cap - size0 : 0;
    const long long stored = kept < room ? kept : room;
    a.counters[0] = size0 + stored;
    a.counters[1] = seen0 + total;
    a.counters[2] += kept - stored;
}

// positions are ordinals here: slots[i] = the bank row of entry i, or -1 when it is not stored
__global__ __launch_bounds__(256) void fk_append_write_kernel(FkAppend a) {
    unsigned pos[FO_ITEMS];
    const unsigned kept = fo_positions(a.counts, pos, [&](int, unsigned i) { return cp_keep(a, i); });
    const long long seen0 = a.header[0], size0 = a.header[1];
    const long long kept0 = fk_ceil_div(seen0, a.every);        // kept rows before this call, had none been lost
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r) {
        const unsigned i = fo_entry(r);
        if (i < a.sel.total) {
            long long slot = -1;
            if (kept & (1u << r)) {
                const long long g = seen0 + pos[r];
                const long long q = g / a.every;
                if (g - q * a.every == 0) slot = size0 + (q - kept0);
            }
            a.slots[i] = (slot >= 0 && slot < a.cap) ? (int)slot : -1;
        }
    }
}

// 16 entries a wave, four lanes an entry: lane group g moves and squares the elements k with (k mod 16) / 4 == g
__global__ __launch_bounds__(256) void fk_append_rows_kernel(FkAppend a) {
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
    const unsigned i = ((unsigned)blockIdx.x * 4 + (unsigned)(tid >> 6)) * 16 + (unsigned)r16;
    const int slot = i < a.sel.total ? a.slots[i] : -1;
    if (!__ballot(slot >= 0)) return;                           // the same for the whole wave
    const char* row = nullptr;
    int cl = -1;
    const bool on = slot >= 0 && fk_keep(a, i, &row, &cl);      // a stored entry is a valid one
    const int bf = a.L.bf16;
    float pp[4] = {0.f, 0.f, 0.f, 0.f};
    float inv = 1.f;
    if (a.normalize) {
        for (int c = 0; c < a.Fp; c += 16)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = c + 4 * g + s;
                const float x = (on && k < a.F) ? fo_ld(row, k, bf) : 0.f;
                pp[s] = pp[s] + x * x;
            }
        inv = fk_inv_norm(fk_tree4x4(pp));
#pragma unroll
        for (int s = 0; s < 4; ++s) pp[s] = 0.f;
    }
    float* dst = a.bank + (long long)(on ? slot : 0) * a.Fp;
    for (int c = 0; c < a.Fp; c += 16) {
        f32x4 v;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = c + 4 * g + s;
            const float x = (on && k < a.F) ? fo_ld(row, k, bf) : 0.f;
            v[s] = a.normalize ? x * inv : x;
            pp[s] = pp[s] + v[s] * v[s];
        }
        if (on) *reinterpret_cast<f32x4*>(dst + c + 4 * g) = v;
    }
    const float n2 = fk_tree4x4(pp);
    if (on && g == 0) { a.norms[slot] = n2; a.bcls[slot] = cl; }
}

// ---- score -------------------------------------------------------------------------------------------------------------------
struct FkScore {
    FoLevels L;
    FoSel sel;
    int F, A;
    int normalize, k, splits;
    unsigned M, steps_per_split;
    const float* bank; const float* norms; const int* cls;
    float* lists; float* bestd; int* besti;                     // workspace: [total][splits][4][k], [total][splits][4] twice
    float* knn; int* index; int* kcls;
};

template <int NT> struct FkGeom {
    static constexpr int FP = 16 * NT, PITCH = FP + 4;
    // two 16-row bank tiles a step (two independent accumulator chains) where both buffers fit in 64 KB of LDS
    static constexpr int TILES = 2 * 32 * (PITCH + 1) * 4 <= 65536 ? 2 : 1;
    static constexpr int TR = 16 * TILES;                       // bank rows per step
    static constexpr int PIECES = TR * FP / 4;                  // 16-byte pieces of a step
    static constexpr int NPRE = (PIECES + 255) / 256;
};

template <int NT, int KL>
__global__ __launch_bounds__(256) void fk_score_kernel(FkScore a) {
    using G = FkGeom<NT>;
    constexpr int FP = G::FP, PITCH = G::PITCH, TILES = G::TILES, TR = G::TR, NPRE = G::NPRE;
    __shared__ __attribute__((aligned(16))) float sh[2 * TR * PITCH];
    __shared__ float nrm[2 * TR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned qi = (unsigned)blockIdx.x * FK_QROWS + (unsigned)wave * 16 + (unsigned)r16;
    // the query row as the B operand: K values 16 kc + 4 g + s of column r16
    Frag<float> fq[NT];
    float qn;
    {
        const char* p = fo_sel_row(a.L, a.sel, a.A, qi);       // null: the query does not count
        float pp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NT; ++kc)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kc * 16 + g * 4 + s;
                const float x = (p && k < a.F) ? fo_ld(p, k, a.L.bf16) : 0.f;
                fq[kc].v[s] = x;
                pp[s] = pp[s] + x * x;
            }
        qn = fk_tree4x4(pp);
        if (a.normalize) {
            const float inv = fk_inv_norm(qn);
#pragma unroll
            for (int s = 0; s < 4; ++s) pp[s] = 0.f;
#pragma unroll
            for (int kc = 0; kc < NT; ++kc)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float v = fq[kc].v[s] * inv;
                    fq[kc].v[s] = v;
                    pp[s] = pp[s] + v * v;
                }
            qn = fk_tree4x4(pp);
        }
    }
    float lst[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) lst[j] = fk_inf();
    float bd = fk_inf();
    int bi = -1;

    const unsigned steps = (a.M + TR - 1) / TR;
    const unsigned s0 = fo_min((unsigned)blockIdx.y * a.steps_per_split, steps), s1 = fo_min(s0 + a.steps_per_split, steps);
    f32x4 pre[NPRE];
    float npre = 0.f;
    auto fetch = [&](unsigned st) {                             // bank rows [st * TR, st * TR + TR) -> registers; zeros beyond M
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int e = u * 256 + tid;
            pre[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < G::PIECES) {
                const unsigned i = st * TR + (unsigned)(e / (FP / 4));
                if (i < a.M) pre[u] = ld_frag<float>(a.bank + (long long)i * FP + (e % (FP / 4)) * 4).v;
            }
        }
        if (tid < TR) { const unsigned i = st * TR + tid; npre = i < a.M ? a.norms[i] : 0.f; }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int e = u * 256 + tid;
            if (e < G::PIECES) *reinterpret_cast<f32x4*>(sh + buf * (TR * PITCH) + (e / (FP / 4)) * PITCH + (e % (FP / 4)) * 4) = pre[u];
        }
        if (tid < TR) nrm[buf * TR + tid] = npre;
    };
    if (s0 < s1) { fetch(s0); stash(0); }
    __syncthreads();
    for (unsigned st = s0; st < s1; ++st) {                     // s0, s1 are the same for the whole workgroup
        const int buf = (int)((st - s0) & 1u);
        if (st + 1 < s1) fetch(st + 1);
        f32x4 acc[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* tile = sh + buf * (TR * PITCH) + r16 * PITCH + g * 4;
#pragma unroll
        for (int kc = 0; kc < NT; ++kc)
#pragma unroll
            for (int t = 0; t < TILES; ++t) mma_chunk(ld_frag<float>(tile + t * 16 * PITCH + kc * 16), fq[kc], acc[t]);
        float d[4 * TILES];
        bool enters = false;
#pragma unroll
        for (int t = 0; t < TILES; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + 4 * g + r;
                const unsigned i = st * TR + (unsigned)row;
                float v = fmaxf((qn + nrm[buf * TR + row]) - 2.f * acc[t][r], 0.f);
                if (i >= a.M) v = fk_inf();
                if (v < bd) { bd = v; bi = (int)i; }              // a lane meets its rows in ascending order: the lower row keeps a tie
                enters = enters || v < lst[KL - 1];
                d[4 * t + r] = v;
            }
        if (__ballot(enters)) {                                 // some lane of the wave has a value for its list (rare once the lists fill)
#pragma unroll
            for (int e = 0; e < 4 * TILES; ++e) {
                float v = d[e];
                if (__ballot(v < lst[KL - 1])) {
#pragma unroll
                    for (int j = 0; j < KL; ++j) {
                        const float lo = v < lst[j] ? v : lst[j], hi = v < lst[j] ? lst[j] : v;
                        lst[j] = lo; v = hi;
                    }
                }
            }
        }
        if (st + 1 < s1) stash(buf ^ 1);
        __syncthreads();
    }
    if (qi < a.sel.total) {
        const long long at = ((long long)qi * a.splits + blockIdx.y) * 4 + g;
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if (j < a.k) a.lists[at * a.k + j] = lst[j];
        a.bestd[at] = bd;
        a.besti[at] = bi;
    }
}

DEV float fk_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}

// a wave per row: lane l owns lists l, l + 64, l + 128, l + 192 of the row's 4 x splits; k_eff rounds take the smallest head away
__global__ __launch_bounds__(256) void fk_merge_kernel(FkScore a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned i = (unsigned)blockIdx.x * 4 + (unsigned)wave;
    if (i >= a.sel.total) return;                               // the same for the whole wave
    const int nl = 4 * a.splits;
    const bool valid = fo_sel_row(a.L, a.sel, a.A, i) != nullptr;
    const float* mine = a.lists + (long long)i * nl * a.k;
    float cur[4];
    int ptr[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int li = lane + 64 * m;
        ptr[m] = 0;
        cur[m] = li < nl ? mine[(long long)li * a.k] : fk_inf();
    }
    const int keff = (unsigned)a.k < a.M ? a.k : (int)a.M;
    float kth = fk_inf();
    for (int round = 0; round < keff; ++round) {
        float head = cur[0];
#pragma unroll
        for (int m = 1; m < 4; ++m) head = cur[m] < head ? cur[m] : head;
        kth = fk_wave_min(head);
        const unsigned long long bal = __ballot(head == kth);
        if (bal && lane == __builtin_ctzll(bal)) {
            bool done = false;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!done && cur[m] == kth) {
                    done = true;
                    ptr[m] += 1;
                    const int li = lane + 64 * m;
                    cur[m] = ptr[m] < a.k ? mine[(long long)li * a.k + ptr[m]] : fk_inf();
                }
            }
        }
    }
    float bd = fk_inf();
    int bi = -1;
    for (int li = lane; li < nl; li += 64) {
        const float d = a.bestd[(long long)i * nl + li];
        const int x = a.besti[(long long)i * nl + li];
        if (d < bd || (d == bd && (unsigned)x < (unsigned)bi)) { bd = d; bi = x; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (od < bd || (od == bd && (unsigned)oi < (unsigned)bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) {
        const bool hit = valid && bi >= 0 && (unsigned)bi < a.M;
        a.knn[i] = valid ? 0.f - kth : 0.f;
        a.index[i] = hit ? bi : -1;
        a.kcls[i] = hit ? a.cls[bi] : -1;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int fk_step_rows(int F) {
    int tr = 0;
    fo_for_width(F, [&](auto nt) { tr = FkGeom<decltype(nt)::value>::TR; });
    return tr;
}

// The split count the library chooses (steps = 0: the bank is not known yet, the most it may choose): one resident set of workgroups,
// as full as whole splits make it - four workgroups a CU up to F = 112, two above (LDS and registers of the wider kernels).  Measured
// on an MI355X (6400 rows, F = 64, 2^20 bank rows): 5 / 7 / 10 / 15 splits take 13.4 / 12.7 / 11.5 / 11.9 ms; 800 rows, F = 224,
// 2^16 bank rows: 19 / 39 / 59 splits take 444 / 340 / 369 us.
int fk_auto_splits(long long rows, int F, long long steps) {
    const long long blocks = (rows + FK_QROWS - 1) / FK_QROWS;
    long long s = (long long)FK_CUS * (F <= 112 ? 4 : 2) / blocks;
    if (s > FK_MAX_SPLITS) s = FK_MAX_SPLITS;
    if (steps > 0 && s > steps) s = steps;
    return (int)(s < 1 ? 1 : s);
}

struct FkLayout { long long header, counts, slots, lists, bestd, besti, total; };

// k = 0: the workspace of append; 1 <= k <= 32: that of score with `splits` (0: the most the library may choose)
bool fk_layout(long long rows, int F, int k, int splits, FkLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS || !fo_width_ok(F) || k < 0 || k > FK_MAX_K || splits < 0 || splits > FK_MAX_SPLITS) return false;
    long long off = 0;
    auto take = [&off](long long bytes) { const long long o = off; off += (bytes + 255) & ~255ll; return o; };
    L->header = L->counts = L->slots = L->lists = L->bestd = L->besti = 0;
    if (k == 0) {
        L->header = take(16);
        L->counts = take(((rows + FO_TILE - 1) / FO_TILE) * 4);
        L->slots = take(rows * 4);
    } else {
        const long long s = splits > 0 ? splits : fk_auto_splits(rows, F, 0);
        L->lists = take(rows * s * 4 * k * 4);
        L->bestd = take(rows * s * 4 * 4);
        L->besti = take(rows * s * 4 * 4);
    }
    L->total = off;
    return true;
}

template <int NT, int KL> void fk_score_launch(hipStream_t st, const FkScore& a) {
    hipLaunchKernelGGL((fk_score_kernel<NT, KL>), dim3((a.sel.total + FK_QROWS - 1) / FK_QROWS, a.splits), dim3(256), 0, st, a);
}
template <int NT> void fk_score_launch_k(hipStream_t st, const FkScore& a) {
    if (a.k == 1) fk_score_launch<NT, 1>(st, a);
    else if (a.k <= 16) fk_score_launch<NT, 16>(st, a);
    else fk_score_launch<NT, 32>(st, a);
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_feature_knn_workspace_bytes(long long rows, int F, int k, int splits) {
    FkLayout L;
    return fk_layout(rows, F, k, splits, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" int effdet_feature_knn_append(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                         const long long* level_batch_strides, const long long* level_cell_strides,
                                         const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                                         const long long* anchor_index, const void* classes, int class_dtype, long long class_pitch,
                                         long long class_stride, long long class_offset, const void* count, int count_is_int64,
                                         int normalize, long long sample_every, long long capacity, float* bank, float* norms,
                                         int* bank_classes, long long* counters, void* workspace, long long workspace_bytes) {
    FkAppend a;
    FkLayout lay;
    if (C < 0 || sample_every < 1 || capacity < 1 || capacity > FK_MAX_CAPACITY) return EFFDET_EINVAL;
    if (!fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.L, &a.sel))
        return EFFDET_EINVAL;
    if (!fo_classes(classes, class_dtype, class_pitch, class_stride, class_offset, C, &a.cls) && C > 0) return EFFDET_EINVAL;
    if (!bank || !norms || !bank_classes || !counters || !workspace) return EFFDET_EINVAL;
    if (!fk_layout((long long)B * K, F, 0, 0, &lay) || workspace_bytes < lay.total) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    char* ws = reinterpret_cast<char*>(workspace);
    a.F = F; a.Fp = (F + 15) & ~15; a.A = A;
    a.normalize = normalize ? 1 : 0; a.every = sample_every; a.cap = capacity;
    a.bank = bank; a.norms = norms; a.bcls = bank_classes; a.counters = counters;
    a.header = reinterpret_cast<long long*>(ws + lay.header);
    a.counts = reinterpret_cast<unsigned*>(ws + lay.counts);
    a.slots = reinterpret_cast<int*>(ws + lay.slots);
    a.nblocks = (a.sel.total + FO_TILE - 1) / FO_TILE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fo_count_kernel<FkAppend>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_base_kernel<FkAppend>, dim3(1), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fk_append_write_kernel, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fk_append_rows_kernel, dim3((a.sel.total + 63) / 64), dim3(256), 0, st, a);
    return effdet_check_launch();
}

extern "C" int effdet_feature_knn_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                        const long long* level_batch_strides, const long long* level_cell_strides,
                                        const long long* level_channel_strides, int F, int A, int B, long long K,
                                        const long long* anchor_index, const void* count, int count_is_int64, int normalize, int k,
                                        int splits, long long M, const float* bank, const float* norms, const int* bank_classes,
                                        float* knn, int* knn_index, int* knn_class, void* workspace, long long workspace_bytes) {
    FkScore a;
    FkLayout lay;
    if (k < 1 || k > FK_MAX_K || splits < 0 || splits > FK_MAX_SPLITS || M < 1 || M > FK_MAX_CAPACITY) return EFFDET_EINVAL;
    if (!fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.L, &a.sel))
        return EFFDET_EINVAL;
    if (!bank || !norms || !bank_classes || !knn || !knn_index || !knn_class || !workspace) return EFFDET_EINVAL;
    const long long rows = (long long)B * K, steps = (M + fk_step_rows(F) - 1) / fk_step_rows(F);
    if (splits == 0) splits = fk_auto_splits(rows, F, steps);
    if (!fk_layout(rows, F, k, splits, &lay) || workspace_bytes < lay.total) return EFFDET_EINVAL;
    EFFDET_ENTER();
    char* ws = reinterpret_cast<char*>(workspace);
    a.F = F; a.A = A;
    a.normalize = normalize ? 1 : 0; a.k = k; a.splits = splits;
    a.M = (unsigned)M; a.steps_per_split = (unsigned)((steps + splits - 1) / splits);
    a.bank = bank; a.norms = norms; a.cls = bank_classes;
    a.lists = reinterpret_cast<float*>(ws + lay.lists);
    a.bestd = reinterpret_cast<float*>(ws + lay.bestd);
    a.besti = reinterpret_cast<int*>(ws + lay.besti);
    a.knn = knn; a.index = knn_index; a.kcls = knn_class;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fo_for_width(F, [&](auto nt) { fk_score_launch_k<decltype(nt)::value>(st, a); });
    hipLaunchKernelGGL(fk_merge_kernel, dim3((a.sel.total + 3) / 4), dim3(256), 0, st, a);
    return effdet_check_launch();
}
