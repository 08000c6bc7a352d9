// Subspace OOD scores on the device: the norm of a pyramid row's component outside the principal subspace of the in-distribution
// features ("residual"), the Mahalanobis distance restricted to those low-variance directions ("partial Mahalanobis", Kamoi &
// Kobayashi 2020) and ViM (Wang et al. 2022), the residual scaled to a logit score's scale and taken off it.
//
//   per row, float32:  xc = f - mu0 (bfloat16 widened exactly),  y = Rt xc  on the float32-input MFMA (16x16x4),
//                      r2 = sum_i y_i^2,  pm = sum_i inv_lambda_i * y_i^2,  r = sqrt(r2),  t = negate ? -logit_score : logit_score
//                      residual = -r,  partial = -pm,  vim = t - alpha * r   (product, then difference: two roundings)
//
//   score      64 (48 at F = 288) rows per workgroup, 16 per wave, xc staged in the wave's LDS rows at pitch Fp + 4 (the geometry and
//              staging of feature_rows.h, shared with feature_ood.hip's score kernel), the product K-chunked by 16 with all
//              Rp / 16 accumulator tiles live, Rt read as 16-byte loads through L2.  With few residual directions a y_i stands alone in the sums, and the rounding of one
//              chain of Fp / 4 accumulations is all of the score's error; the accumulator registers that few tiles leave free then
//              hold S = 4 (Rp / 16 <= NT / 4) or 2 (<= NT / 2) independent chains over the K-chunks kc = s mod S, added as
//              (c0 + c1) + (c2 + c3) at the end - no more registers than S = 1 with all tiles, half the rounding error at S = 4.
//              A lane holds y_i for i = 16 t + (lane & 15) of rows 4 (lane >> 4) + 0 .. 3; the two sums run over t ascending in
//              the lane and then over the 16 lanes of a row by the xor tree 1, 2, 4, 8 - a fixed order that depends on nothing
//              but Rp, so a row's bits do not depend on which rows share its wave or its workgroup.
//   calibrate  the same staging and the same device function for r; a workgroup adds its valid rows' t and r in (b, j) order to
//              one float64 partial, and one workgroup adds the partials in workgroup order (a contiguous run per thread, then a
//              fixed tree) to the running sums.  Rows that do not count add nothing, so no compaction pass is needed to fix the
//              order.  No floating-point atomics.
//
// Every row index is compared with the level table before a pointer is formed, every store index with its extent before the
// store; no call synchronises with the host or allocates, so all of them can be captured in a graph.
#include "common.h"
#include "feature_rows.h"

namespace {

struct FsArgs {
    FoLevels L;
    FoSel sel;
    int F, A, RT;                                               // RT = Rp / 16 tiles of residual directions
    const float *Rt, *inv_lambda, *mu0;                         // [Rp][Fp], [Rp], [Fp]; zero in the padding
    const float* ls; long long ls_pitch, ls_stride; int negate; // the logit score [B, K] (strided) or null
    float alpha;
    float *residual, *partial, *vim;                            // score
    double* part; unsigned nblocks;                             // calibrate: [nblocks][3] = {n, sum t, sum r} per workgroup
    long long* counters; double* sums;                          // calibrate: the running n and {sum t, sum r}
};

constexpr int FS_MIN_ROWS = 48;                                 // the fewest rows of a workgroup at any width

// K-chains of the product for RT tiles of residual directions at NT tiles of width: as many as the accumulators of NT tiles hold
constexpr int fs_chains(int NT, int RT) { return 4 * RT <= NT ? 4 : (2 * RT <= NT ? 2 : 1); }

// r[q], pm[q] of row 4 * (lane >> 4) + q of the wave's 16 staged rows, in every lane of the row; RT <= NT / S
template <int NT, int S> DEV void fs_rows(const FsArgs& a, const float* xs, int lane, float (&r)[4], float (&pm)[4]) {
    constexpr int FP = FoRowGeom<NT>::FP, PITCH = FoRowGeom<NT>::PITCH, TM = NT / S;
    const int r16 = lane & 15, g = lane >> 4;
    const int RT = a.RT;                                        // uniform: the tile tests below are scalar branches
    f32x4 ch[S][TM];
#pragma unroll
    for (int c = 0; c < S; ++c)
#pragma unroll
        for (int t = 0; t < TM; ++t) ch[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kc0 = 0; kc0 < NT; kc0 += S) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const int kc = kc0 + c;
            if (kc < NT) {
                const Frag<float> fa = ld_frag<float>(xs + r16 * PITCH + kc * 16 + g * 4);
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    if (t < RT) {
                        const Frag<float> fb = ld_frag<float>(a.Rt + (long long)(t * 16 + r16) * FP + kc * 16 + g * 4);
                        mma_chunk(fa, fb, ch[c][t]);
                    }
                }
            }
        }
    }
    f32x4 (&acc)[TM] = ch[0];
    if constexpr (S == 2) {
#pragma unroll
        for (int t = 0; t < TM; ++t) acc[t] = ch[0][t] + ch[1][t];
    }
    if constexpr (S == 4) {
#pragma unroll
        for (int t = 0; t < TM; ++t) acc[t] = (ch[0][t] + ch[1][t]) + (ch[2][t] + ch[3][t]);
    }
    float s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { s[q] = 0.f; pm[q] = 0.f; }
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        if (t < RT) {
            const float il = a.inv_lambda ? a.inv_lambda[t * 16 + r16] : 0.f;       // (null in calibrate, which uses r alone)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y2 = acc[t][q] * acc[t][q];
                s[q] += y2;
                pm[q] += il * y2;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[q] += __shfl_xor(s[q], o, 64);
            pm[q] += __shfl_xor(pm[q], o, 64);
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = sqrtf(s[q]);
}

// the logit score of entry i after the sign rule
DEV float fs_logit(const FsArgs& a, unsigned i) {
    const unsigned b = i / a.sel.K, j = i - b * a.sel.K;
    const float v = a.ls[(long long)b * a.ls_pitch + (long long)j * a.ls_stride];
    return a.negate ? -v : v;
}

template <int NT, int S>
__global__ __launch_bounds__(FoRowGeom<NT>::WAVES * 64) void fs_score_kernel(FsArgs a) {
    constexpr int PITCH = FoRowGeom<NT>::PITCH, WAVES = FoRowGeom<NT>::WAVES;
    __shared__ __attribute__((aligned(16))) float sh[16 * WAVES * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned row0 = (unsigned)blockIdx.x * (16 * WAVES) + (unsigned)wave * 16;
    float* xs = sh + wave * 16 * PITCH;
    const unsigned valid = fo_stage_centered<NT>(a.L, a.sel, a.A, a.F, a.mu0, row0, xs, lane);
    __syncthreads();
    float r[4], pm[4];
    fs_rows<NT, S>(a, xs, lane, r, pm);
    if (r16 == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned i = row0 + 4 * g + q;
            if (i < a.sel.total) {
                const bool v = (valid >> (4 * g + q)) & 1u;
                a.residual[i] = v ? -r[q] : 0.f;
                a.partial[i] = v ? -pm[q] : 0.f;
                if (a.vim) {
                    float out = 0.f;
                    if (v) {
                        const float ar = a.alpha * r[q];
                        out = fs_logit(a, i) - ar;
                    }
                    a.vim[i] = out;
                }
            }
        }
    }
}

// part[workgroup] = {n, sum t, sum r} over the workgroup's valid rows in (b, j) order
template <int NT, int S>
__global__ __launch_bounds__(FoRowGeom<NT>::WAVES * 64) void fs_calib_kernel(FsArgs a) {
    constexpr int PITCH = FoRowGeom<NT>::PITCH, WAVES = FoRowGeom<NT>::WAVES, ROWS = FoRowGeom<NT>::ROWS;
    __shared__ __attribute__((aligned(16))) float sh[16 * WAVES * PITCH];
    __shared__ float rt[ROWS], rr[ROWS];
    __shared__ unsigned rv[ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const unsigned row0 = (unsigned)blockIdx.x * ROWS + (unsigned)wave * 16;
    float* xs = sh + wave * 16 * PITCH;
    const unsigned valid = fo_stage_centered<NT>(a.L, a.sel, a.A, a.F, a.mu0, row0, xs, lane);
    __syncthreads();
    float r[4], pm[4];
    fs_rows<NT, S>(a, xs, lane, r, pm);
    if (r16 == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int w = wave * 16 + 4 * g + q;
            const bool v = (valid >> (4 * g + q)) & 1u;
            rv[w] = v ? 1u : 0u;
            rr[w] = v ? r[q] : 0.f;
            rt[w] = v ? fs_logit(a, row0 + 4 * g + q) : 0.f;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double st = 0.0, sr = 0.0;
        unsigned n = 0;
        for (int w = 0; w < ROWS; ++w) {
            if (rv[w]) { ++n; st += (double)rt[w]; sr += (double)rr[w]; }
        }
        double* o = a.part + 3ll * blockIdx.x;
        o[0] = (double)n; o[1] = st; o[2] = sr;
    }
}

// one workgroup: the partials in workgroup order (a contiguous run per thread, then the tree of fo_block_sum) -> the running sums
__global__ __launch_bounds__(256) void fs_calib_reduce_kernel(FsArgs a) {
    __shared__ double sh[FO_THREADS];
    const int tid = threadIdx.x;
    const unsigned chunk = (a.nblocks + FO_THREADS - 1) / FO_THREADS;
    const unsigned lo = fo_min((unsigned)tid * chunk, a.nblocks), hi = fo_min(lo + chunk, a.nblocks);
    double n = 0.0, st = 0.0, sr = 0.0;                         // n <= 2^27: exact in float64
    for (unsigned k = lo; k < hi; ++k) { n += a.part[3ll * k]; st += a.part[3ll * k + 1]; sr += a.part[3ll * k + 2]; }
    n = fo_block_sum<double>(n, sh, tid);
    st = fo_block_sum<double>(st, sh, tid);
    sr = fo_block_sum<double>(sr, sh, tid);
    if (tid == 0) { a.counters[0] += (long long)n; a.sums[0] += st; a.sums[1] += sr; }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
long long fs_workspace(long long rows) {
    if (rows < 1 || rows > FO_MAX_ROWS) return EFFDET_EINVAL;
    return (((rows + FS_MIN_ROWS - 1) / FS_MIN_ROWS) * 24 + 255) & ~255ll;
}

template <int NT> void fs_score_launch(hipStream_t st, const FsArgs& a) {
    const dim3 grid((a.sel.total + FoRowGeom<NT>::ROWS - 1) / FoRowGeom<NT>::ROWS), block(FoRowGeom<NT>::WAVES * 64);
    switch (fs_chains(NT, a.RT)) {
        case 4: hipLaunchKernelGGL((fs_score_kernel<NT, 4>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((fs_score_kernel<NT, 2>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((fs_score_kernel<NT, 1>), grid, block, 0, st, a); break;
    }
}
template <int NT> void fs_calib_launch(hipStream_t st, FsArgs& a) {
    a.nblocks = (a.sel.total + FoRowGeom<NT>::ROWS - 1) / FoRowGeom<NT>::ROWS;
    const dim3 grid(a.nblocks), block(FoRowGeom<NT>::WAVES * 64);
    switch (fs_chains(NT, a.RT)) {                              // the chains of the score: r agrees bit for bit
        case 4: hipLaunchKernelGGL((fs_calib_kernel<NT, 4>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((fs_calib_kernel<NT, 2>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((fs_calib_kernel<NT, 1>), grid, block, 0, st, a); break;
    }
    hipLaunchKernelGGL(fs_calib_reduce_kernel, dim3(1), dim3(FO_THREADS), 0, st, a);
}

// the arguments both entry points share; false: refuse
bool fs_args(int dtype, int num_levels, const void* const* bases, const long long* cells, const long long* batch_strides,
             const long long* cell_strides, const long long* channel_strides, int F, int A, int B, long long K,
             const long long* anchor_index, const void* count, int count_is_int64, const float* Rt, const float* mu0, int Rp,
             const float* logit_score, long long ls_pitch, long long ls_stride, int negate, FsArgs* a) {
    if (!fo_feature_rows(dtype, num_levels, bases, cells, batch_strides, cell_strides, channel_strides, F, A, B, K, anchor_index, count,
                         count_is_int64, &a->L, &a->sel))
        return false;
    if (!Rt || !mu0 || Rp < 16 || Rp % 16 != 0 || Rp > (F + 15) / 16 * 16) return false;
    if (logit_score && (ls_pitch < 0 || ls_stride < 0)) return false;
    a->F = F; a->A = A; a->RT = Rp / 16;
    a->Rt = Rt; a->inv_lambda = nullptr; a->mu0 = mu0;
    a->ls = logit_score; a->ls_pitch = ls_pitch; a->ls_stride = ls_stride; a->negate = negate ? 1 : 0;
    a->alpha = 0.f;
    a->residual = a->partial = a->vim = nullptr;
    a->part = nullptr; a->nblocks = 0; a->counters = nullptr; a->sums = nullptr;
    return true;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" long long effdet_feature_subspace_workspace_bytes(long long rows) { return fs_workspace(rows); }

extern "C" int effdet_feature_subspace_score(void* stream, int dtype, int num_levels, const void* const* level_bases,
                                             const long long* level_cells, const long long* level_batch_strides,
                                             const long long* level_cell_strides, const long long* level_channel_strides, int F, int A,
                                             int B, long long K, const long long* anchor_index, const void* count, int count_is_int64,
                                             const float* Rt, const float* inv_lambda, const float* mu0, int Rp,
                                             const float* logit_score, long long ls_pitch, long long ls_stride, int negate, float alpha,
                                             float* residual, float* partial, float* vim) {
    FsArgs a;
    if (!fs_args(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B, K,
                 anchor_index, count, count_is_int64, Rt, mu0, Rp, logit_score, ls_pitch, ls_stride, negate, &a))
        return EFFDET_EINVAL;
    if (!inv_lambda || !residual || !partial || (vim && !logit_score)) return EFFDET_EINVAL;
    EFFDET_ENTER();                                              // (the refusals above are pure host code)
    a.inv_lambda = inv_lambda; a.alpha = alpha;
    a.residual = residual; a.partial = partial; a.vim = vim;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fo_for_width(F, [&](auto nt) { fs_score_launch<decltype(nt)::value>(st, a); });
    return effdet_check_launch();
}

extern "C" int effdet_feature_subspace_calibrate(void* stream, int dtype, int num_levels, const void* const* level_bases,
                                                 const long long* level_cells, const long long* level_batch_strides,
                                                 const long long* level_cell_strides, const long long* level_channel_strides, int F,
                                                 int A, int B, long long K, const long long* anchor_index, const void* count,
                                                 int count_is_int64, const float* Rt, const float* mu0, int Rp, const float* logit_score,
                                                 long long ls_pitch, long long ls_stride, int negate, long long* counters, double* sums,
                                                 void* workspace, long long workspace_bytes) {
    FsArgs a;
    if (!fs_args(dtype, num_levels, level_bases, level_cells, level_batch_strides, level_cell_strides, level_channel_strides, F, A, B, K,
                 anchor_index, count, count_is_int64, Rt, mu0, Rp, logit_score, ls_pitch, ls_stride, negate, &a))
        return EFFDET_EINVAL;
    if (!logit_score || !counters || !sums || !workspace || workspace_bytes < fs_workspace((long long)B * K)) return EFFDET_EINVAL;
    EFFDET_ENTER();
    a.part = reinterpret_cast<double*>(workspace); a.counters = counters; a.sums = sums;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    fo_for_width(F, [&](auto nt) { fs_calib_launch<decltype(nt)::value>(st, a); });
    return effdet_check_launch();
}
