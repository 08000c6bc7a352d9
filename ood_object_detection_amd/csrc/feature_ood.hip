// Feature-space OOD scores on the device: the class-conditional Gaussian (Mahalanobis) distance with a tied covariance and its
// "relative" form over rows of the BiFPN pyramid.
//
//   fit     a batch's rows -> the running float64 statistics n_c (int64), s_c = sum f, S = sum f f^T:
//           compaction of the valid rows in (b, j) order (compact.h), then S as per-workgroup partials over fixed row chunks
//           that one launch adds in a fixed order to the running matrix, then s_c / n_c by one workgroup per class that walks
//           the compacted rows in order.  Products of float32 values are exact in float64; only the order of the additions is a choice, and it
//           depends on nothing but the number of valid rows.
//   score   64 (48 at F = 288) rows per workgroup, 16 per wave: xc = f - mu_0 staged in LDS, z0 = W_0 xc and z = W xc on the
//           float32-input MFMA (16x16x4) with the factors read through L2 in K-chunks of 16, z written back over the wave's own
//           LDS rows as the A operand of the F x C product with the whitened class means.
//
// Row selection, class labels, the level table of the features and the staging of xc are feature_rows.h's.  Every row index is
// compared with the table before a pointer is formed, every store index with its extent before the store; no call synchronises
// with the host or allocates, so all of them can be captured in a graph.
#include "common.h"
#include "feature_rows.h"

namespace {

constexpr int FO_MAX_CLASSES = 1024;
constexpr int FO_CHUNKS = 16;                                   // row chunks of the scatter-matrix partials
constexpr int FO_ST = 16;                                       // S tile: 16 x 16 entries, one per thread
constexpr int FO_SROWS = 32;                                    // rows staged per step of the S kernel
constexpr int FO_CROWS = 256;                                   // rows looked at per step of the class-sum kernel

// ---- fit ---------------------------------------------------------------------------------------------------------------------
struct FoRec { unsigned rowcell; int cls; };                    // b * P + cell, class

struct FoFit {
    FoLevels L;
    FoSel sel;
    FoClasses cls;
    int F, A;
    unsigned* counts; unsigned nblocks;                         // kept entries per compaction workgroup, then bases
    unsigned* header;                                           // [0] = number of valid rows of this call
    FoRec* list; unsigned cap;
    double* partial;                                            // [FO_CHUNKS][F][F]
    long long* n_c; double* s_c; double* S;
};

// is entry i = b * K + j a valid row?
DEV bool fo_keep(const FoFit& a, unsigned i, FoRec* rec) {
    unsigned b; long long an;
    if (!fo_select(a.sel, i, &b, &an)) return false;
    const int cl = fo_class(a.cls, b, i - b * a.sel.K);
    if (cl < 0) return false;
    rec->rowcell = b * a.L.P + (unsigned)(an / a.A);
    rec->cls = cl;
    return true;
}
DEV bool cp_keep(const FoFit& a, unsigned i) { FoRec rec; return fo_keep(a, i, &rec); }
DEV unsigned cp_begin(const FoFit&) { return 0u; }
DEV void cp_finish(const FoFit& a, unsigned, unsigned total) { a.header[0] = fo_min(total, a.cap); }

__global__ __launch_bounds__(256) void fo_fit_write_kernel(FoFit a) {
    FoRec rec[FO_ITEMS];
    unsigned pos[FO_ITEMS];
    const unsigned kept = fo_positions(a.counts, pos, [&](int r, unsigned i) {
        rec[r].rowcell = 0; rec[r].cls = 0;
        return fo_keep(a, i, &rec[r]);
    });
#pragma unroll
    for (int r = 0; r < FO_ITEMS; ++r)
        if ((kept & (1u << r)) && pos[r] < a.cap) a.list[pos[r]] = rec[r];
}

// blockIdx.x = S tile (ti, tj), blockIdx.y = row chunk: partial[chunk][i][j] = sum over the chunk's rows of f_i f_j, rows in order
__global__ __launch_bounds__(256) void fo_fit_scatter_kernel(FoFit a) {
    __shared__ float xs[FO_SROWS][2 * FO_ST];
    __shared__ const char* rowp[FO_SROWS];
    const int tid = threadIdx.x;
    const int T = (a.F + FO_ST - 1) / FO_ST;
    const int ti = blockIdx.x / T, tj = blockIdx.x - ti * T;
    const unsigned n = fo_min(a.header[0], a.cap);
    const unsigned chunk = (n + FO_CHUNKS - 1) / FO_CHUNKS;
    const unsigned lo = fo_min((unsigned)blockIdx.y * chunk, n), hi = fo_min(lo + chunk, n);
    const int i = tid >> 4, j = tid & 15;
    double acc = 0.0;
    for (unsigned r0 = lo; r0 < hi; r0 += FO_SROWS) {           // lo, hi are the same for the whole workgroup
        if (tid < FO_SROWS) {
            const unsigned r = r0 + tid;
            const char* p = nullptr;
            if (r < hi) {
                const unsigned rc = a.list[r].rowcell;
                const unsigned b = rc / a.L.P;
                p = fo_row(a.L, b, rc - b * a.L.P);
            }
            rowp[tid] = p;
        }
        __syncthreads();
        for (int e = tid; e < FO_SROWS * 2 * FO_ST; e += FO_THREADS) {
            const int row = e >> 5, col = e & 31;
            const int f = col < FO_ST ? ti * FO_ST + col : tj * FO_ST + col - FO_ST;
            const char* p = rowp[row];
            xs[row][col] = (p && f < a.F) ? fo_ld(p, f, a.L.bf16) : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < FO_SROWS; ++r) acc += (double)xs[r][i] * (double)xs[r][FO_ST + j];
        __syncthreads();
    }
    const int fi = ti * FO_ST + i, fj = tj * FO_ST + j;
    if (fi < a.F && fj < a.F) a.partial[((long long)blockIdx.y * a.F + fi) * a.F + fj] = acc;
}

// S[e] += the chunks' partials in chunk order
__global__ __launch_bounds__(256) void fo_fit_reduce_kernel(FoFit a) {
    const long long e = (long long)blockIdx.x * FO_THREADS + threadIdx.x, FF = (long long)a.F * a.F;
    if (e >= FF) return;
    double s = 0.0;
    for (int c = 0; c < FO_CHUNKS; ++c) s += a.partial[(long long)c * FF + e];
    a.S[e] += s;
}

// workgroup c: s_c[c] += sum of the rows of class c in row order, n_c[c] += their number.  The workgroup looks at 256 rows a step;
// the waves' ballots say which of them belong to the class, and only those are walked (in row order, by every thread alike).
__global__ __launch_bounds__(256) void fo_fit_class_kernel(FoFit a) {
    __shared__ const char* rowp[FO_CROWS];
    __shared__ unsigned long long match[FO_THREADS / 64];
    __shared__ unsigned shc[FO_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x;
    const unsigned n = fo_min(a.header[0], a.cap);
    const int f0 = tid, f1 = tid + FO_THREADS;
    double acc0 = 0.0, acc1 = 0.0;
    unsigned mine = 0;
    for (unsigned r0 = 0; r0 < n; r0 += FO_CROWS) {
        const unsigned r = r0 + tid;
        const char* p = nullptr;
        if (r < n) {
            const FoRec rec = a.list[r];
            if (rec.cls == c) {
                const unsigned b = rec.rowcell / a.L.P;
                p = fo_row(a.L, b, rec.rowcell - b * a.L.P);
                ++mine;
            }
        }
        rowp[tid] = p;
        const unsigned long long bal = __ballot(p != nullptr);
        if (lane == 0) match[wave] = bal;
        __syncthreads();
        for (int w = 0; w < FO_THREADS / 64; ++w) {
            for (unsigned long long m = match[w]; m; m &= m - 1) {     // the same for the whole workgroup
                const char* q = rowp[w * 64 + __builtin_ctzll(m)];
                if (f0 < a.F) acc0 += (double)fo_ld(q, f0, a.L.bf16);
                if (f1 < a.F) acc1 += (double)fo_ld(q, f1, a.L.bf16);
            }
        }
        __syncthreads();
    }
    const unsigned cnt = fo_block_sum<unsigned>(mine, shc, tid);
    if (cnt == 0) return;
    if (f0 < a.F) a.s_c[(long long)c * a.F + f0] += acc0;
    if (f1 < a.F) a.s_c[(long long)c * a.F + f1] += acc1;
    if (tid == 0) a.n_c[c] += (long long)cnt;
}

// ---- score -------------------------------------------------------------------------------------------------------------------
struct FoScore {
    FoLevels L;
    FoSel sel;
    int F, Cp, A;                                               // Cp: C rounded up to 32
    const float *W, *W0, *M, *m2, *mu0;                         // [Fp][Fp], [Fp][Fp], [Cp][Fp], [Cp], [Fp]; Fp = F rounded up to 16
    float* maha; float* rel; int* nearest;
};

// acc[t] = the wave's 16 rows (xs, LDS) times rows [16 t, 16 t + 16) of Wm ([.][FP] in global memory), K = FP
template <int NT> DEV void fo_gemm(const float* xs, const float* Wm, int lane, f32x4 (&acc)[NT]) {
    constexpr int FP = FoRowGeom<NT>::FP, PITCH = FoRowGeom<NT>::PITCH;
    const int r16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kc = 0; kc < NT; ++kc) {
        const Frag<float> fa = ld_frag<float>(xs + r16 * PITCH + kc * 16 + g * 4);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const Frag<float> fb = ld_frag<float>(Wm + (long long)(t * 16 + r16) * FP + kc * 16 + g * 4);
            mma_chunk(fa, fb, acc[t]);
        }
    }
}

// per-row sum of squares of a [16 rows][FP] product held as NT accumulator tiles: s[r] = row 4 * (lane >> 4) + r, in every lane
template <int NT> DEV void fo_row_sumsq(const f32x4 (&acc)[NT], float (&s)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += acc[t][r] * acc[t][r];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += __shfl_xor(s[r], o, 64);
}

template <int NT>
__global__ __launch_bounds__(FoRowGeom<NT>::WAVES * 64) void fo_score_kernel(FoScore a) {
    constexpr int FP = FoRowGeom<NT>::FP, PITCH = FoRowGeom<NT>::PITCH, WAVES = FoRowGeom<NT>::WAVES;
    __shared__ __attribute__((aligned(16))) float sh[16 * WAVES * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned row0 = (unsigned)blockIdx.x * (16 * WAVES) + (unsigned)wave * 16;
    float* xs = sh + wave * 16 * PITCH;
    const unsigned valid = fo_stage_centered<NT>(a.L, a.sel, a.A, a.F, a.mu0, row0, xs, lane);
    __syncthreads();
    f32x4 acc[NT];
    float d0[4], q[4];
    fo_gemm<NT>(xs, a.W0, lane, acc);
    fo_row_sumsq<NT>(acc, d0);
    fo_gemm<NT>(xs, a.W, lane, acc);
    fo_row_sumsq<NT>(acc, q);
    __syncthreads();                                            // every read of xc is done: z takes its place
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) xs[(4 * g + r) * PITCH + t * 16 + r16] = acc[t][r];
    __syncthreads();
    float best[4];
    int bi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { best[r] = __builtin_inff(); bi[r] = -1; }
    for (int ct = 0; ct < a.Cp; ct += 32) {                     // two class tiles a step: two independent accumulator chains
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
        const float* m0 = a.M + (long long)(ct + r16) * FP + g * 4;
        const float* m1 = m0 + 16ll * FP;
#pragma unroll 2
        for (int kc = 0; kc < NT; ++kc) {
            const Frag<float> fa = ld_frag<float>(xs + r16 * PITCH + kc * 16 + g * 4);
            mma_chunk(fa, ld_frag<float>(m0 + kc * 16), c0);
            mma_chunk(fa, ld_frag<float>(m1 + kc * 16), c1);
        }
        const float n0 = a.m2[ct + r16], n1 = a.m2[ct + 16 + r16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e0 = (q[r] - 2.f * c0[r]) + n0;
            if (e0 < best[r]) { best[r] = e0; bi[r] = ct + r16; }
            const float e1 = (q[r] - 2.f * c1[r]) + n1;
            if (e1 < best[r]) { best[r] = e1; bi[r] = ct + 16 + r16; }
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float od = __shfl_xor(best[r], o, 64);
            const int oi = __shfl_xor(bi[r], o, 64);
            if (od < best[r] || (od == best[r] && (unsigned)oi < (unsigned)bi[r])) { best[r] = od; bi[r] = oi; }
        }
    if (r16 == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned i = row0 + 4 * g + r;
            if (i < a.sel.total) {
                const bool v = (valid >> (4 * g + r)) & 1u;
                a.maha[i] = v ? -best[r] : 0.f;
                a.rel[i] = v ? -(best[r] - d0[r]) : 0.f;
                a.nearest[i] = v ? bi[r] : -1;
            }
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct FoLayout { long long header, counts, list, partial, total; };

bool fo_layout(long long rows, int F, FoLayout* L) {
    if (rows < 1 || rows > FO_MAX_ROWS || !fo_width_ok(F)) return false;
    long long off = 0;
    auto take = [&off](long long bytes) { const long long o = off; off += (bytes + 255) & ~255ll; return o; };
    L->header = take(16);
    L->counts = take(((rows + FO_TILE - 1) / FO_TILE) * 4);
    L->list = take(rows * (long long)sizeof(FoRec));
    L->partial = take((long long)FO_CHUNKS * F * F * 8);
    L->total = off;
    return true;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_feature_ood_workspace_bytes(long long rows, int F) {
    FoLayout L;
    return fo_layout(rows, F, &L) ? L.total : (long long)EFFDET_EINVAL;
}

extern "C" int effdet_feature_ood_fit(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                      const long long* level_batch_strides, const long long* level_cell_strides,
                                      const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                                      const long long* anchor_index, const void* classes, int class_dtype, long long class_pitch,
                                      long long class_stride, long long class_offset, const void* count, int count_is_int64,
                                      long long* n_c, double* s_c, double* S, void* workspace, long long workspace_bytes) {
    FoFit a;
    FoLayout lay;
    if (C < 1 || C > FO_MAX_CLASSES || !n_c || !s_c || !S || !workspace) return EFFDET_EINVAL;
    if (!fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.L, &a.sel) ||
        !fo_classes(classes, class_dtype, class_pitch, class_stride, class_offset, C, &a.cls))
        return EFFDET_EINVAL;
    if (!fo_layout((long long)B * K, F, &lay) || workspace_bytes < lay.total) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    char* ws = reinterpret_cast<char*>(workspace);
    a.F = F; a.A = A;
    a.header = reinterpret_cast<unsigned*>(ws + lay.header);
    a.counts = reinterpret_cast<unsigned*>(ws + lay.counts);
    a.nblocks = (a.sel.total + FO_TILE - 1) / FO_TILE;
    a.list = reinterpret_cast<FoRec*>(ws + lay.list); a.cap = a.sel.total;
    a.partial = reinterpret_cast<double*>(ws + lay.partial);
    a.n_c = n_c; a.s_c = s_c; a.S = S;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int T = (F + FO_ST - 1) / FO_ST;
    hipLaunchKernelGGL(fo_count_kernel<FoFit>, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_base_kernel<FoFit>, dim3(1), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_fit_write_kernel, dim3(a.nblocks), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_fit_scatter_kernel, dim3(T * T, FO_CHUNKS), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_fit_reduce_kernel, dim3((F * F + FO_THREADS - 1) / FO_THREADS), dim3(FO_THREADS), 0, st, a);
    hipLaunchKernelGGL(fo_fit_class_kernel, dim3(C), dim3(FO_THREADS), 0, st, a);
    return effdet_check_launch();
}

extern "C" int effdet_feature_ood_score(void* stream, int dtype, int num_levels, const void* const* level_bases, const long long* level_cells,
                                        const long long* level_batch_strides, const long long* level_cell_strides,
                                        const long long* level_channel_strides, int F, int C, int A, int B, long long K,
                                        const long long* anchor_index, const void* count, int count_is_int64, const float* W,
                                        const float* W0, const float* M, const float* m2, const float* mu0, float* mahalanobis,
                                        float* relative, int* nearest) {
    FoScore a;
    if (C < 1 || C > FO_MAX_CLASSES ||
        !fo_feature_rows(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B,
                         K, anchor_index, count, count_is_int64, &a.L, &a.sel))
        return EFFDET_EINVAL;
    if (!W || !W0 || !M || !m2 || !mu0 || !mahalanobis || !relative || !nearest) return EFFDET_EINVAL;
    EFFDET_ENTER();
    a.F = F; a.Cp = (C + 31) & ~31; a.A = A;
    a.W = W; a.W0 = W0; a.M = M; a.m2 = m2; a.mu0 = mu0;
    a.maha = mahalanobis; a.rel = relative; a.nearest = nearest;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fo_for_width(F, [&](auto nt) {
        using G = FoRowGeom<decltype(nt)::value>;
        hipLaunchKernelGGL(fo_score_kernel<decltype(nt)::value>, dim3((a.sel.total + G::ROWS - 1) / G::ROWS), dim3(G::WAVES * 64), 0, st, a);
    });
    return effdet_check_launch();
}
