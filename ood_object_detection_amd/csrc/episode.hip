// The few-shot episode stage between the MetaHead's outputs and the novelty score (infer.py:362-447 projection phase, :566-654
// meta phase), float32 throughout: discrete decisions are taken on these numbers, so nothing here uses bf16 or the matrix cores.
//
//   effdet_episode_select    per (image, level): the `keep` most confident anchors (what `res_conf > quantile(res_conf, 0.875)`
//                            keeps, :380-394), as ascending (y, x, a) indices.  One workgroup streams the level's confidences from
//                            global memory (an 80 x 80 level is 230 KB, more than the LDS): three radix passes over the 32-bit
//                            order-preserving key with the histogram in LDS find the keep-th largest key, one more walk compacts
//                            with an order-preserving block scan.  Ties at the cut go to the lower index.
//   effdet_episode_feed      the ProjectionNet feed rows of the kept anchors, [embedding | anchor enc | level enc | cell enc | 0..]
//                            (:366-378), copied (never recomputed) from the activations and the three encoding tables.
//   effdet_episode_cluster   normalise, one prototype per image, valid prototypes, re-pick, similarity of every row to the
//                            prototypes, target (:423-447 / :605-654) without any n x n matrix.  With e the normalised rows,
//                            s = sigmoid(dot_mult (conf + dot_add)), g = sum_j s_j e_j:
//                                weighted_sim.mean(2)[i]              = s_i (e_i . g) / n
//                                sim_mat[:, P_valid].mean(1)[i]       = e_i . mean_v e_pv
//                                weighted_sim[:, :, P_valid].sum(2)[i] = s_i (e_i . sum_v s_pv e_pv)
//                                init_cluster.mean(1)[i]              = e_pi . mean_j e_pj
//                            Seven short launches, as the data dependencies ask: (a) norms, s, partials of g; (a') g; (b) scores
//                            and per-image argmax in parts; (c) prototype stage in one workgroup; (d) second argmax; (c') second
//                            prototype stage; (e) E P^T with max / argmax / mean epilogue, prototypes in LDS, E read once.
//                            Every reduction runs in a fixed order (per-wave partials, then a sequential second stage): results
//                            are bitwise reproducible.  argmax ties go to the lower index.
#include "episode_rows.h"

namespace {

constexpr int EP_MAX_LEVELS = 8;
constexpr int EP_MAX_G = 256;             // the cluster stage's cap on rows_split

// order-preserving key of a float; -0 counts as +0, as torch's comparison does
DEV unsigned int ep_key(float f) {
    const unsigned int u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelLevel { const float* conf; long long stride; int N; int keep; int* out; };
struct SelArgs { SelLevel lv[EP_MAX_LEVELS]; };

__global__ __launch_bounds__(1024) void episode_select_kernel(SelArgs args) {
    const SelLevel L = args.lv[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = L.conf + (long long)b * L.stride;
    int* out = L.out + (long long)b * L.keep;
    const int N = L.N, keep = L.keep;
    if (keep >= N) {                                               // levels of at most 4 x 4 cells keep every anchor (:381-382)
        for (int i = tid; i < N; i += 1024) out[i] = i;
        return;
    }
    __shared__ unsigned int h[2048];
    __shared__ unsigned int part[1024];
    __shared__ unsigned int sel[2];
    __shared__ unsigned int wsum[2][16];
    // ---- the keep-th largest key T and the number of keys above it (11 + 11 + 10 bits, most significant first)
    unsigned int prefix = 0, c_hi = 0;
    int bits_done = 0;
    for (int pass = 0; pass < 3; ++pass) {
        const int bits = pass < 2 ? 11 : 10;
        const int shift = 32 - bits_done - bits;
        const unsigned int mask = (1u << bits) - 1u;
        for (int i = tid; i < 2048; i += 1024) h[i] = 0;
        __syncthreads();
        for (int i = tid; i < N; i += 1024) {
            const unsigned int key = ep_key(row[i]);
            if (bits_done == 0 || (key >> (32 - bits_done)) == prefix) atomicAdd(&h[(key >> shift) & mask], 1u);
        }
        __syncthreads();
        // thread t owns bins 2t, 2t + 1; suffix sums from the top over the per-thread totals
        const unsigned int l0 = h[2 * tid], l1 = h[2 * tid + 1], sown = l0 + l1;
        unsigned int incl = sown;
        part[tid] = incl;
        __syncthreads();
#pragma unroll
        for (int off = 1; off < 1024; off <<= 1) {
            const unsigned int add = tid + off < 1024 ? part[tid + off] : 0u;
            __syncthreads();
            incl += add;
            part[tid] = incl;
            __syncthreads();
        }
        const unsigned int need = (unsigned int)keep - c_hi;
        const unsigned int above = incl - sown;
        if (above < need && above + sown >= need) {                 // exactly one thread
            if (above + l1 >= need) { sel[0] = 2 * tid + 1; sel[1] = above; }
            else { sel[0] = 2 * tid; sel[1] = above + l1; }
        }
        __syncthreads();
        prefix = (prefix << bits) | sel[0];
        c_hi += sel[1];
        bits_done += bits;
        __syncthreads();
    }
    const unsigned int T = prefix;
    const unsigned int need_eq = (unsigned int)keep - c_hi;         // >= 1: that many keys equal to T are kept, lowest indices first
    // ---- order-preserving compaction, 1024 anchors per step
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned int base_gt = 0, base_eq = 0;
    int buf = 0;
    for (int c0 = 0; c0 < N; c0 += 1024, buf ^= 1) {
        const int i = c0 + tid;
        const unsigned int key = ep_key(row[i < N ? i : N - 1]);
        const bool gt = i < N && key > T, eq = i < N && key == T;
        const unsigned long long mg = __ballot(gt), me = __ballot(eq);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) wsum[buf][wave] = (unsigned int)__popcll(mg) | ((unsigned int)__popcll(me) << 16);
        __syncthreads();
        unsigned int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const unsigned int v = wsum[buf][w]; total += v; if (w < wave) before += v; }
        const unsigned int gt_ex = base_gt + (before & 0xFFFFu) + (unsigned int)__popcll(mg & below);
        const unsigned int eq_ex = base_eq + (before >> 16) + (unsigned int)__popcll(me & below);
        const bool take = gt || (eq && eq_ex < need_eq);
        const unsigned int pos = gt_ex + (eq_ex < need_eq ? eq_ex : need_eq);
        if (take && pos < (unsigned int)keep) out[pos] = i;
        base_gt += total & 0xFFFFu;
        base_eq += total >> 16;
    }
}

struct FeedLevel { const float* act; long long act_stride; const float* conf; long long conf_stride; const int* sel; int keep; int roff; int W; };
struct FeedArgs { FeedLevel lv[EP_MAX_LEVELS]; int nl; };

__global__ __launch_bounds__(256) void episode_feed_kernel(FeedArgs a, const float* anch, const float* lev, const float* cell,
                                                           int first_level, int A, int F, int Kp, int R, long long rows, int vec,
                                                           float* feed, float* conf_out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long gr = (long long)blockIdx.x * 4 + wave; gr < rows; gr += (long long)gridDim.x * 4) {
        const int b = (int)(gr / R), r = (int)(gr % R);
        int l = 0;
        while (l + 1 < a.nl && r >= a.lv[l + 1].roff) ++l;
        const FeedLevel L = a.lv[l];
        const int W = L.W, N = A * W * W;
        int idx = L.sel[(long long)b * L.keep + (r - L.roff)];
        idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);                // a foreign index never leaves the level
        const int an = idx % A, cid = idx / A, y = cid / W, x = cid % W;
        const float* src = L.act + (long long)b * L.act_stride + (long long)cid * F;
        float* dst = feed + gr * Kp;
        if (vec) {
            for (int c = lane; c < (F >> 2); c += 64) reinterpret_cast<f32x4*>(dst)[c] = reinterpret_cast<const f32x4*>(src)[c];
        } else {
            for (int c = lane; c < F; c += 64) dst[c] = src[c];
        }
        for (int t = lane; t < Kp - F; t += 64) {
            float v = 0.f;
            if (t < 8) v = anch[an * 8 + t];
            else if (t < 14) v = lev[(first_level + l) * 6 + (t - 8)];
            else if (t < 42) {
                // the reference's expression (:370-371): L[j] = cell_enc[y] for j < W, cell_enc[j - W] for j >= W; cell (y, x)
                // gets [L[2x] | L[2x + 1]]
                const int u = t - 14, half = u >= 14 ? 1 : 0, e = u - 14 * half, j = 2 * x + half;
                v = cell[(j < W ? y : j - W) * 14 + e];
            }
            dst[F + t] = v;
        }
        if (lane == 0) conf_out[gr] = L.conf[(long long)b * L.conf_stride + idx];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// cluster
// ---------------------------------------------------------------------------------------------------------------------------

// (a) inv[i] = 1 / max(||x_i||, 1e-12), s[i], gpart[block] = sum over the block's rows of s_i e_i
__global__ __launch_bounds__(256) void episode_prep_kernel(const float* X, const float* confs, int n, int d, int rows_per_block,
                                                           float dot_mult, float dot_add, const float* dots,
                                                           float* inv, float* s, float* gpart) {
    __shared__ float red[4][64 * PL_MAX_DL];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PlDots dt = pl_dots(dots, dot_mult, dot_add);
    int r1;
    const int r0 = pl_row_range(rows_per_block, n, r1);
    float acc[PL_MAX_DL];
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) acc[k] = 0.f;
    for (int i = r0 + wave; i < r1; i += 4) {
        float v[PL_MAX_DL];
        const float iv = pl_load_row(X + (long long)i * d, d, lane, v);
        const float si = pl_sigmoid(dt.m * (confs[i] + dt.a));
#pragma unroll
        for (int k = 0; k < PL_MAX_DL; ++k) acc[k] += si * (v[k] * iv);
        if (lane == 0) { inv[i] = iv; s[i] = si; }
    }
#pragma unroll
    for (int k = 0; k < PL_MAX_DL; ++k) red[wave][lane + 64 * k] = acc[k];
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) gpart[(long long)blockIdx.x * d + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// (a') g[c] = sum_k gpart[k][c], in order
// (64 columns per workgroup; wave w sums the partials k = w, w + 4, ... with eight loads in flight, then the four sums in order)
__global__ __launch_bounds__(256) void episode_gsum_kernel(const float* gpart, int G, int d, float* g) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + lane, cc = c < d ? c : d - 1;
    float t = 0.f;
    for (int k0 = wave; k0 < G; k0 += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + 4 * u; v[u] = gpart[(long long)(k < G ? k : G - 1) * d + cc]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) t += k0 + 4 * u < G ? v[u] : 0.f;
    }
    red[wave][lane] = t;
    __syncthreads();
    if (wave == 0 && c < d) g[c] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// (b) / (d): score_i = s_i (e_i . v); best row of the part (blockIdx.x) of image blockIdx.y, ties to the lower row
__global__ __launch_bounds__(256) void episode_score_kernel(const float* X, const float* inv, const float* s, const float* v, int p, int d,
                                                            int per, float* best_s, int* best_i) {
    __shared__ float vl[64 * PL_MAX_DL];
    __shared__ float bs[4];
    __shared__ int bi[4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int c = threadIdx.x; c < 64 * PL_MAX_DL; c += 256) vl[c] = c < d ? v[c] : 0.f;
    __syncthreads();
    const int img = blockIdx.y;
    const int j0 = blockIdx.x * per;
    int j1 = j0 + per; if (j1 > p) j1 = p;
    float best = -INFINITY;
    int arg = j0 < j1 ? j0 : 0x7fffffff;
    for (int j = j0 + wave; j < j1; j += 4) {
        const long long i = (long long)img * p + j;
        const float* row = X + i * d;
        float dot = 0.f;
        for (int c = lane; c < d; c += 64) dot += row[c] * vl[c];
        dot = wave_reduce_sum(dot);
        const float sc = s[i] * (inv[i] * dot);
        if (sc > best) { best = sc; arg = j; }                      // rows ascend within a wave: the first of equals stays
    }
    if (lane == 0) { bs[wave] = best; bi[wave] = arg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bs[w] > best || (bs[w] == best && bi[w] < arg)) { best = bs[w]; arg = bi[w]; }
        best_s[img * gridDim.x + blockIdx.x] = best;
        best_i[img * gridDim.x + blockIdx.x] = arg;
    }
}

// (c) / (c'): one workgroup.  stage 0: proto0, avg_init0, valid, n_valid, cmean = mean_v e_pv, vsum = sum_v s_pv e_pv.
//             stage 1: proto, avg_init, target_clust[j] = e_pj . cmean.
__global__ __launch_bounds__(1024) void episode_proto_kernel(const float* X, const float* inv, const float* s, const float* best_s,
                                                             const int* best_i, int parts, int p, int d, int m, int stage,
                                                             int use_thresh, float thresh, float* cmean, float* vsum,
                                                             long long* proto_out, float* avg_out, unsigned char* valid_out,
                                                             int* n_valid_out, float* tclust_out) {
    __shared__ long long pidx[PL_MAX_M];
    __shared__ float vec[64 * PL_MAX_DL];
    __shared__ float avg[PL_MAX_M];
    __shared__ int val[PL_MAX_M];
    __shared__ int nv_;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < m) {
        float best = best_s[tid * parts];
        int arg = best_i[tid * parts];
        for (int q = 1; q < parts; ++q) {
            const float b2 = best_s[tid * parts + q];
            const int a2 = best_i[tid * parts + q];
            if (b2 > best || (b2 == best && a2 < arg)) { best = b2; arg = a2; }
        }
        if (arg < 0 || arg >= p) arg = 0;
        pidx[tid] = (long long)tid * p + arg;
        proto_out[tid] = pidx[tid];
    }
    __syncthreads();
    // vec = sum_j e_pj  (then avg_i = e_pi . vec / m - 1 / m, the row means of init_cluster)
    for (int c = tid; c < d; c += 1024) {
        float t = 0.f;
        for (int j = 0; j < m; ++j) t += X[pidx[j] * d + c] * inv[pidx[j]];
        vec[c] = t;
    }
    __syncthreads();
    for (int i = wave; i < m; i += 16) {
        const float* row = X + pidx[i] * d;
        const float iv = inv[pidx[i]];
        float dot = 0.f;
        for (int c = lane; c < d; c += 64) dot += (row[c] * iv) * vec[c];
        dot = wave_reduce_sum(dot);
        if (lane == 0) { avg[i] = dot / (float)m - 1.0f / (float)m; avg_out[i] = avg[i]; }
    }
    __syncthreads();
    if (stage == 0) {
        if (tid == 0) {
            float mean = 0.f;
            for (int i = 0; i < m; ++i) mean += avg[i];
            mean /= (float)m;
            const float thr = use_thresh ? thresh : mean;
            int nv = 0;
            for (int i = 0; i < m; ++i) { val[i] = avg[i] > thr ? 1 : 0; nv += val[i]; valid_out[i] = (unsigned char)val[i]; }
            nv_ = nv; n_valid_out[0] = nv;
        }
        __syncthreads();
        const float nvf = (float)nv_;
        for (int c = tid; c < d; c += 1024) {
            float t = 0.f, u = 0.f;
            for (int j = 0; j < m; ++j) {
                const float e = X[pidx[j] * d + c] * inv[pidx[j]];
                if (val[j]) { t += e; u += s[pidx[j]] * e; }
            }
            cmean[c] = t / nvf;                                     // an empty valid set gives NaN, as the reference's mean does
            vsum[c] = u;
        }
    } else {
        for (int c = tid; c < d; c += 1024) vec[c] = cmean[c];
        __syncthreads();
        for (int i = wave; i < m; i += 16) {
            const float* row = X + pidx[i] * d;
            const float iv = inv[pidx[i]];
            float dot = 0.f;
            for (int c = lane; c < d; c += 64) dot += (row[c] * iv) * vec[c];
            dot = wave_reduce_sum(dot);
            if (lane == 0) tclust_out[i] = dot;
        }
    }
}

// (e) the arithmetic of novelty_score_kernel (postprocess.hip): normalised prototypes in LDS, a wave per row; 16 waves share one
// copy of the prototypes (at 2 048 workgroups of 4 waves filling the LDS copies read more than E itself)
constexpr int EP_ASSIGN_WAVES = 16;
__global__ __launch_bounds__(64 * EP_ASSIGN_WAVES) void episode_assign_kernel(const float* X, const float* inv, const float* s, const long long* proto,
                                                             const float* tclust, int n, int d, int m, int use_max,
                                                             float* sim, long long* nearest, float* target) {
    extern __shared__ float pl_[];                     // [m][d]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int j = wave; j < m; j += EP_ASSIGN_WAVES) {
        const long long pj = proto[j];
        const float* row = X + pj * (long long)d;
        const float iv = inv[pj];
        for (int c = lane; c < d; c += 64) pl_[j * d + c] = row[c] * iv;
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * EP_ASSIGN_WAVES + wave; i < n; i += (long long)gridDim.x * EP_ASSIGN_WAVES) {
        const float* row = X + i * d;
        const float iv = inv[i];
        float xv[PL_MAX_DL];                                        // the normalised row, read once
#pragma unroll
        for (int k = 0; k < PL_MAX_DL; ++k) { const int c = lane + 64 * k; xv[k] = (c < d ? row[c] : 0.f) * iv; }
        float acc_sum = 0.f, acc_max = -INFINITY;
        int arg = 0;
        for (int j = 0; j < m; ++j) {
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < PL_MAX_DL; ++k) { const int c = lane + 64 * k; if (c < d) dot += xv[k] * pl_[j * d + c]; }
            dot = wave_reduce_sum(dot);
            acc_sum += dot;
            if (dot > acc_max) { acc_max = dot; arg = j; }
        }
        if (lane == 0) {
            if (use_max) { sim[i] = acc_max; nearest[i] = arg; target[i] = s[i] * tclust[arg] * acc_max; }
            else { const float sv = acc_sum / (float)m; sim[i] = sv; nearest[i] = -1; target[i] = s[i] * sv; }
        }
    }
}

struct ClusterPlan { int G, rows_per_block, parts, per, p; long long o_inv, o_gpart, o_g, o_cmean, o_vsum, o_bs, o_bi, total; };
ClusterPlan cluster_plan(int n, int d, int m) {
    ClusterPlan c;
    c.p = n / m;
    const RowsSplit r = rows_split(n, EP_MAX_G);
    c.G = r.G; c.rows_per_block = r.rows_per_block;
    c.parts = (c.p + 63) / 64; if (c.parts > PL_MAX_PARTS) c.parts = PL_MAX_PARTS; if (c.parts < 1) c.parts = 1;
    c.per = (c.p + c.parts - 1) / c.parts;
    long long o = 0;
    c.o_inv = o; o += n;
    c.o_gpart = o; o += (long long)c.G * d;
    c.o_g = o; o += d;
    c.o_cmean = o; o += d;
    c.o_vsum = o; o += d;
    c.o_bs = o; o += (long long)m * c.parts;
    c.o_bi = o; o += (long long)m * c.parts;
    c.total = o;
    return c;
}
bool cluster_shape_ok(int n, int d, int m) {
    return pl_shape_ok(n, d, m) && n % m == 0;
}

}  // namespace

extern "C" int effdet_episode_select(void* stream, int B, int num_levels, const void* const* confs, const long long* image_strides,
                                     const int* counts, const int* keeps, void* const* outs) {
    EFFDET_ENTER();
    if (B <= 0 || num_levels <= 0 || num_levels > EP_MAX_LEVELS || !confs || !image_strides || !counts || !keeps || !outs) return EFFDET_EINVAL;
    SelArgs a{};
    for (int l = 0; l < num_levels; ++l) {
        if (!confs[l] || !outs[l] || counts[l] <= 0 || keeps[l] <= 0 || keeps[l] > counts[l] || image_strides[l] < counts[l]) return EFFDET_EINVAL;
        a.lv[l] = SelLevel{static_cast<const float*>(confs[l]), image_strides[l], counts[l], keeps[l], static_cast<int*>(outs[l])};
    }
    hipLaunchKernelGGL(episode_select_kernel, dim3(B, num_levels), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), a);
    return effdet_check_launch();
}

extern "C" int effdet_episode_feed(void* stream, int B, int num_levels, const void* const* activs, const long long* activ_strides,
                                   const void* const* confs, const long long* conf_strides, const void* const* sels, const int* keeps,
                                   const int* widths, const float* anch_enc, const float* lev_enc, int lev_rows, const float* cell_enc,
                                   int cell_rows, int first_level, int A, int F, int Kp, float* feed, float* conf_out) {
    EFFDET_ENTER();
    if (B <= 0 || num_levels <= 0 || num_levels > EP_MAX_LEVELS || !activs || !activ_strides || !confs || !conf_strides || !sels || !keeps ||
        !widths || !anch_enc || !lev_enc || !cell_enc || !feed || !conf_out || A <= 0 || A > 9 || F <= 0 || Kp < F + 42 ||
        first_level < 0 || first_level + num_levels > lev_rows)
        return EFFDET_EINVAL;
    FeedArgs a{};
    a.nl = num_levels;
    int R = 0, vec = (F % 4 == 0 && Kp % 4 == 0 && reinterpret_cast<uintptr_t>(feed) % 16 == 0) ? 1 : 0;
    for (int l = 0; l < num_levels; ++l) {
        const int W = widths[l];
        if (!activs[l] || !confs[l] || !sels[l] || W <= 0 || W > cell_rows || keeps[l] <= 0 || keeps[l] > A * W * W ||
            activ_strides[l] < (long long)W * W * F || conf_strides[l] < (long long)W * W * A)
            return EFFDET_EINVAL;
        if (reinterpret_cast<uintptr_t>(activs[l]) % 16 != 0 || activ_strides[l] % 4 != 0) vec = 0;
        a.lv[l] = FeedLevel{static_cast<const float*>(activs[l]), activ_strides[l], static_cast<const float*>(confs[l]), conf_strides[l],
                            static_cast<const int*>(sels[l]), keeps[l], R, W};
        R += keeps[l];
    }
    const long long rows = (long long)B * R;
    long long blocks = (rows + 3) / 4; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(episode_feed_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, anch_enc, lev_enc,
                       cell_enc, first_level, A, F, Kp, R, rows, vec, feed, conf_out);
    return effdet_check_launch();
}

extern "C" long long effdet_episode_cluster_workspace_floats(int n, int d, int m) {
    if (!cluster_shape_ok(n, d, m)) return -1;
    return cluster_plan(n, d, m).total;
}

extern "C" int effdet_episode_cluster(void* stream, const float* embds, const float* confs, int n, int d, int m, float dot_mult,
                                      float dot_add, const float* dots, int use_thresh, float valid_threshold, int use_max,
                                      float* workspace, long long workspace_floats, float* soft_thresh, long long* proto0,
                                      float* avg_init0, unsigned char* valid, int* n_valid, long long* proto, float* avg_init,
                                      float* target_clust, float* sim, long long* nearest, float* target) {
    EFFDET_ENTER();
    if (!embds || !confs || !workspace || !soft_thresh || !proto0 || !avg_init0 || !valid || !n_valid || !proto || !avg_init ||
        !target_clust || !sim || !nearest || !target || !cluster_shape_ok(n, d, m))
        return EFFDET_EINVAL;
    const ClusterPlan c = cluster_plan(n, d, m);
    if (workspace_floats < c.total) return EFFDET_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* inv = workspace + c.o_inv; float* gpart = workspace + c.o_gpart; float* g = workspace + c.o_g;
    float* cmean = workspace + c.o_cmean; float* vsum = workspace + c.o_vsum; float* bs = workspace + c.o_bs;
    int* bi = reinterpret_cast<int*>(workspace + c.o_bi);
    hipLaunchKernelGGL(episode_prep_kernel, dim3(c.G), dim3(256), 0, st, embds, confs, n, d, c.rows_per_block, dot_mult, dot_add, dots,
                       inv, soft_thresh, gpart);
    hipLaunchKernelGGL(episode_gsum_kernel, dim3((d + 63) / 64), dim3(256), 0, st, gpart, c.G, d, g);
    hipLaunchKernelGGL(episode_score_kernel, dim3(c.parts, m), dim3(256), 0, st, embds, inv, soft_thresh, g, c.p, d, c.per, bs, bi);
    hipLaunchKernelGGL(episode_proto_kernel, dim3(1), dim3(1024), 0, st, embds, inv, soft_thresh, bs, bi, c.parts, c.p, d, m, 0, use_thresh,
                       valid_threshold, cmean, vsum, proto0, avg_init0, valid, n_valid, target_clust);
    hipLaunchKernelGGL(episode_score_kernel, dim3(c.parts, m), dim3(256), 0, st, embds, inv, soft_thresh, vsum, c.p, d, c.per, bs, bi);
    hipLaunchKernelGGL(episode_proto_kernel, dim3(1), dim3(1024), 0, st, embds, inv, soft_thresh, bs, bi, c.parts, c.p, d, m, 1, use_thresh,
                       valid_threshold, cmean, vsum, proto, avg_init, valid, n_valid, target_clust);
    int blocks = (n + EP_ASSIGN_WAVES - 1) / EP_ASSIGN_WAVES; if (blocks > 512) blocks = 512;
    hipLaunchKernelGGL(episode_assign_kernel, dim3(blocks), dim3(64 * EP_ASSIGN_WAVES), (size_t)m * d * 4, st, embds, inv, soft_thresh, proto, target_clust,
                       n, d, m, use_max, sim, nearest, target);
    return effdet_check_launch();
}
