// The projection phase's episode losses (infer.py:448-498, summed at :787-789) on the decisions effdet_episode_cluster took,
// forward and backward, float32 throughout and without any n x n matrix.  With e the normalised rows, l = dot_mult (conf + dot_add),
// s = sigmoid(l), P_k = e[proto_k], cmean the mean of the valid first prototypes and cls the task class:
//     target_clust[k] = P_k . cmean                                 sim_mat[:, max_idxs[valid]].mean(1)[max_idxs]
//     sim_i           = e_i . P[nearest_i]  ('max')                 all_max_sims_clust
//                     = e_i . mean_k P_k    ('avg')                 all_avg_sims_clust
//     y_k             = labs[proto_k] == cls                        sim_target[max_idxs, max_idxs] == 1
//     t_i             = labs[0] == cls && labs[nearest_i] == cls    gather(sim_target, 1, all_max_idxs.reshape(1, -1)) == 1: ROW 0 of the
//                                                                   matrix and COLUMN nearest_i, a value in [0, m) - the reference's
//                                                                   behaviour, kept as it is
//                     = labs[i] == cls      ('avg')
//     cosine_loss(x, t) = mean(max(0, t ? 1 - x : x - margin)), a term whose argument is exactly 0 passes gradient
//     'separate': clust = cos(target_clust, y), embds = cos(s sim, t)      'same': clust = 0, embds = cos(s sim target_clust[nearest], t)
//     'no_conf':  clust = cos(target_clust, y), embds = cos(sim, t)        'avg':  clust = 0, embds = cos(s sim, t)
//     inner_target = s target_clust[nearest] sim ('max') / s sim ('avg');  obj = sum_i max(l, 0) - l [labs_i > -1] + log1p(exp(-|l|))
//
// Forward, three launches: (1) one workgroup: P, cmean, mean_k P_k, target_clust, clust_loss; (2) a wave per row over a fixed split
// of the rows: inv, s, sim (kept for the backward), inner_target, per-block partials of the two sums and the nine group
// statistics; (3) one wave adds the partials in order.
// Backward, three launches: (1) a wave per row: dsim_i, dl_i, dconf_i, dE_i = (dsim_i P[nearest_i] - e_i dsim_i sim_i) inv_i and
// per-block partials of d dot_mult / d dot_add; (2) grid (part, prototype), pl_part_kernel of episode_rows.h: a workgroup walks its
// part of the rows and adds dsim_i e_i of the rows whose nearest prototype is its own, in ascending row order, into registers -
// [parts][m][d] partials, no atomics;
// (3) one workgroup: dP_k = sum over the parts + dtarget_clust_k cmean, dcmean = sum_k dtarget_clust_k P_k, both taken through the
// normalisation into the rows proto_k / proto0_k one after the other (a row can be both, and an ordinary row too), and the two
// dot sums.  Every reduction has a fixed order: two calls give the same bits.
//
// Indices come from the caller: proto / proto0 are clamped into [0, n) and nearest into [0, m) before use, so a bad index gives a
// wrong number, never an out-of-range access.
#include "episode_rows.h"

namespace {

constexpr int PL_NPART = 12;              // hinge sum, obj sum, 3 group sums, task min, other max, no-obj max, (pad), 3 counts

enum { PL_SEPARATE = 0, PL_SAME = 1, PL_NO_CONF = 2 };

// the hinge's input
DEV float pl_x(int use_max, int mode, float s, float sim, float tcn) {
    if (!use_max || mode == PL_SEPARATE) return s * sim;
    if (mode == PL_SAME) return (s * sim) * tcn;
    return sim;
}

DEV float pl_hinge_arg(bool t, float x, float margin) { return t ? 1.0f - x : x - margin; }

struct PlPlan {
    RowsSplit rows;
    PartsSplit parts;
    PlKept kept;                                                                          // from the forward for the backward
    long long o_fpart, o_rowc, o_dotpart, o_dPpart, o_bTpart, o_dP, total;                // scratch
};
PlPlan pl_plan(int n, int d, int m) {
    PlPlan p;
    p.rows = rows_split(n, PL_MAX_G);
    p.parts = parts_split(n, PL_MAX_PARTS);
    long long o = pl_kept(n, d, m, p.kept);
    p.o_fpart = o; o += (long long)p.rows.G * PL_NPART;
    p.o_rowc = o; o += 4LL * n;
    p.o_dotpart = o; o += (long long)p.rows.G * 2;
    p.o_dPpart = o; o += (long long)p.parts.parts * m * d;
    p.o_bTpart = o; o += 2LL * p.parts.parts * m;
    p.o_dP = o; o += (long long)m * d;
    p.total = o;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------

// (1) one workgroup: the prototype stage (P, cmean, pmean, tc, nv), then losses[0] = clust_loss
__global__ __launch_bounds__(1024) void pl_proto_kernel(const float* X, const long long* labs, int n, int d, int m, long long cls_id,
                                                        const long long* cls_dev, const long long* proto0, const unsigned char* valid,
                                                        const long long* proto, int use_max, int mode, float margin, float* P,
                                                        float* cmean, float* pmean, float* tc, float* nv_out, float* losses) {
    __shared__ PlProtoLds L;
    pl_proto_stage(L, X, n, d, m, proto0, valid, proto, P, cmean, pmean, tc, nv_out);
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        if (use_max && mode != PL_SAME) {
            const long long cls = cls_dev ? cls_dev[0] : cls_id;
            for (int k = 0; k < m; ++k) {
                const bool y = labs[pl_clamp(proto[k], n)] == cls;
                const float arg = pl_hinge_arg(y, L.tc[k], margin);
                sum += arg < 0.f ? 0.f : arg;                       // NaN stays NaN, as torch's clamp keeps it
            }
            sum /= (float)m;
        }
        losses[0] = sum;
    }
}

// (2) a wave per row
__global__ __launch_bounds__(256) void pl_rows_kernel(const float* X, const float* confs, const long long* labs, int n, int d, int m,
                                                      int rows_per_block, long long cls_id, const long long* cls_dev, float dot_mult,
                                                      float dot_add, const float* dots, const long long* nearest, int use_max, int mode,
                                                      float margin, const float* P, const float* pmean, const float* tc, float* inv,
                                                      float* s, float* sim, float* inner_target, float* fpart) {
    __shared__ float red[4][PL_NPART];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PlDots dt = pl_dots(dots, dot_mult, dot_add);
    const long long cls = cls_dev ? cls_dev[0] : cls_id;
    const bool lab0 = labs[0] == cls;
    int r1;
    const int r0 = pl_row_range(rows_per_block, n, r1);
    float hs = 0.f, os = 0.f, g_sum[3] = {0.f, 0.f, 0.f}, t_min = INFINITY, o_max = -INFINITY, n_max = -INFINITY;
    int g_cnt[3] = {0, 0, 0};
    for (int i = r0 + wave; i < r1; i += 4) {
        float v[PL_MAX_DL];
        const float iv = pl_load_row(X + (long long)i * d, d, lane, v);
        const float l = dt.m * (confs[i] + dt.a);
        const float si = pl_sigmoid(l);
        const int k = pl_nearest(nearest, i, m, use_max);
        float tcn = 0.f;
        const float* prow = pl_proto_row(k, d, P, pmean, tc, tcn);
        const long long lab = labs[i];
        const bool t = use_max ? lab0 && labs[k] == cls : lab == cls;
        const float dot = pl_row_dot(v, iv, prow, d, lane);
        const float arg = pl_hinge_arg(t, pl_x(use_max, mode, si, dot, tcn), margin);
        hs += arg < 0.f ? 0.f : arg;
        const float tobj = lab > -1 ? 1.f : 0.f;
        os += (fmaxf(l, 0.f) - l * tobj) + log1pf(expf(-fabsf(l)));
        const float it = use_max ? (si * tcn) * dot : si * dot;
        if (lab == cls) { g_sum[0] += it; t_min = fminf(t_min, it); ++g_cnt[0]; }
        else if (lab > -1) { g_sum[1] += it; o_max = fmaxf(o_max, it); ++g_cnt[1]; }
        else if (lab == -1) { g_sum[2] += it; n_max = fmaxf(n_max, it); ++g_cnt[2]; }
        if (lane == 0) { inv[i] = iv; s[i] = si; sim[i] = dot; inner_target[i] = it; }
    }
    if (lane == 0) {
        float* r = red[wave];
        r[0] = hs; r[1] = os; r[2] = g_sum[0]; r[3] = g_sum[1]; r[4] = g_sum[2]; r[5] = t_min; r[6] = o_max; r[7] = n_max; r[8] = 0.f;
        r[9] = __int_as_float(g_cnt[0]); r[10] = __int_as_float(g_cnt[1]); r[11] = __int_as_float(g_cnt[2]);
    }
    __syncthreads();
    if (threadIdx.x < PL_NPART) {
        const int j = threadIdx.x;
        float o;
        if (j < 5 || j == 8) o = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
        else if (j == 5) o = fminf(fminf(red[0][j], red[1][j]), fminf(red[2][j], red[3][j]));
        else if (j < 8) o = fmaxf(fmaxf(red[0][j], red[1][j]), fmaxf(red[2][j], red[3][j]));
        else o = __int_as_float(__float_as_int(red[0][j]) + __float_as_int(red[1][j]) + __float_as_int(red[2][j]) + __float_as_int(red[3][j]));
        fpart[(long long)blockIdx.x * PL_NPART + j] = o;
    }
}

// (3) one wave: the G partials in a fixed order
__global__ __launch_bounds__(64) void pl_final_kernel(const float* fpart, int G, int n, float* losses, float* stats, int* counts) {
    const int lane = threadIdx.x;
    float sum[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, t_min = INFINITY, o_max = -INFINITY, n_max = -INFINITY;
    int cnt[3] = {0, 0, 0};
    for (int b = lane; b < G; b += 64) {
        const float* p = fpart + (long long)b * PL_NPART;
#pragma unroll
        for (int j = 0; j < 5; ++j) sum[j] += p[j];
        t_min = fminf(t_min, p[5]); o_max = fmaxf(o_max, p[6]); n_max = fmaxf(n_max, p[7]);
#pragma unroll
        for (int j = 0; j < 3; ++j) cnt[j] += __float_as_int(p[9 + j]);
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) sum[j] = wave_reduce_sum(sum[j]);
    t_min = -wave_reduce_max(-t_min); o_max = wave_reduce_max(o_max); n_max = wave_reduce_max(n_max);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        for (int o = 32; o > 0; o >>= 1) cnt[j] += __shfl_xor(cnt[j], o, 64);
    if (lane == 0) {
        losses[1] = sum[0] / (float)n;
        losses[2] = sum[1];
        const float ext[3] = {t_min, o_max, n_max};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float mean = sum[2 + j] / (float)cnt[j];           // an empty group: 0 / 0 = NaN
            stats[2 * j] = mean;
            stats[2 * j + 1] = mean != mean ? mean : ext[j];         // empty, or a NaN member (fmin / fmax would drop it)
            counts[j] = cnt[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------------------------

// (1) a wave per row: dconf, the row's own part of dE, and for the part kernel rowc[4 i] = dsim_i inv_i, rowc[4 i + 2] = the row's
// dtarget_clust contribution
__global__ __launch_bounds__(256) void pl_bwd_rows_kernel(const float* X, const float* confs, const long long* labs, int n, int d, int m,
                                                          int rows_per_block, long long cls_id, const long long* cls_dev,
                                                          float dot_mult, float dot_add, const float* dots, const long long* nearest,
                                                          int use_max, int mode, float margin, const float* gup, const float* P,
                                                          const float* pmean, const float* tc, const float* inv, const float* s,
                                                          const float* sim, float* dE, float* dconf, float* rowc, float* dotpart) {
    __shared__ float red[4][2];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const PlDots dt = pl_dots(dots, dot_mult, dot_add);
    const long long cls = cls_dev ? cls_dev[0] : cls_id;
    const bool lab0 = labs[0] == cls;
    const float ge = gup[1], go = gup[2];
    int r1;
    const int r0 = pl_row_range(rows_per_block, n, r1);
    float pm = 0.f, pa = 0.f;
    for (int i = r0 + wave; i < r1; i += 4) {
        const float* row = X + (long long)i * d;
        float v[PL_MAX_DL];
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; v[q] = c < d ? row[c] : 0.f; }
        const float iv = inv[i], si = s[i], simi = sim[i], cf = confs[i];
        const int k = pl_nearest(nearest, i, m, use_max);
        float tcn = 0.f;
        const float* prow = pl_proto_row(k, d, P, pmean, tc, tcn);
        const long long lab = labs[i];
        const bool t = use_max ? lab0 && labs[k] == cls : lab == cls;
        const float arg = pl_hinge_arg(t, pl_x(use_max, mode, si, simi, tcn), margin);
        const float dx = arg >= 0.f ? (t ? -ge : ge) / (float)n : 0.f;
        float dsim, ds, dtcr = 0.f;
        if (!use_max || mode == PL_SEPARATE) { dsim = dx * si; ds = dx * simi; }
        else if (mode == PL_SAME) { dsim = (dx * si) * tcn; ds = (dx * simi) * tcn; dtcr = dx * (si * simi); }
        else { dsim = dx; ds = 0.f; }
        const float tobj = lab > -1 ? 1.f : 0.f;
        const float dl = ds * (si * (1.0f - si)) + go * (si - tobj);
        pm += dl * (cf + dt.a);
        pa += dl * dt.m;
        const float edot = dsim * simi;                              // e_i . de_i
        float* out = dE + (long long)i * d;
#pragma unroll
        for (int q = 0; q < PL_MAX_DL; ++q) { const int c = lane + 64 * q; if (c < d) out[c] = (dsim * prow[c] - (v[q] * iv) * edot) * iv; }
        if (lane == 0) { dconf[i] = dl * dt.m; rowc[4LL * i] = dsim * iv; rowc[4LL * i + 2] = dtcr; }   // pl_part_kernel<false>'s two slots
    }
    if (lane == 0) { red[wave][0] = pm; red[wave][1] = pa; }
    __syncthreads();
    if (threadIdx.x < 2) dotpart[(long long)blockIdx.x * 2 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// (2) is pl_part_kernel<false, float> of episode_rows.h: dPpart [parts][m][d], bTpart [parts][m][2] with the dtarget_clust sums in slot 0

// (3) one workgroup: the prototype gradients, through the normalisation into dE's rows; d dot_mult, d dot_add
__global__ __launch_bounds__(1024) void pl_bwd_proto_kernel(const float* X, const long long* labs, int n, int d, int m, int parts, int G,
                                                            long long cls_id, const long long* cls_dev, const long long* proto0,
                                                            const unsigned char* valid, const long long* proto, int use_max, int mode,
                                                            float margin, const float* gup, const float* P, const float* cmean,
                                                            const float* tc, const float* nv_in, const float* inv, const float* dPpart,
                                                            const float* bTpart, const float* dotpart, float* dP, float* dE, float* ddots) {
    __shared__ float dcmv[64 * PL_MAX_DL];
    __shared__ float dtc[PL_MAX_M], dotP[PL_MAX_M], dot0[PL_MAX_M];
    __shared__ long long rr[PL_MAX_M], rr0[PL_MAX_M];
    __shared__ int val[PL_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < m) {
        const int k = tid;
        const long long r = pl_clamp(proto[k], n);
        float g = 0.f;
        if (use_max && mode != PL_SAME) {
            const long long cls = cls_dev ? cls_dev[0] : cls_id;
            const bool y = labs[r] == cls;
            const float arg = pl_hinge_arg(y, tc[k], margin);
            g = arg >= 0.f ? (y ? -gup[0] : gup[0]) / (float)m : 0.f;
        } else if (use_max) {
            for (int q = 0; q < parts; ++q) g += bTpart[2 * ((long long)q * m + k)];
        }
        dtc[k] = g; rr[k] = r; rr0[k] = pl_clamp(proto0[k], n); val[k] = valid[k] ? 1 : 0;
    }
    __syncthreads();
    const int md = m * d;
    for (int idx = tid; idx < md; idx += 1024) {
        const int k = idx / d, c = idx - k * d;
        float t = 0.f;
        if (use_max) {
            for (int q = 0; q < parts; ++q) t += dPpart[((long long)q * m + k) * d + c];
        } else {
            for (int q = 0; q < parts; ++q) t += dPpart[(long long)q * d + c];
            t /= (float)m;
        }
        dP[idx] = t + dtc[k] * cmean[c];
    }
    const float nvf = nv_in[0];
    for (int c = tid; c < d; c += 1024) {
        float t = 0.f;
        for (int k = 0; k < m; ++k) t += dtc[k] * P[(long long)k * d + c];
        dcmv[c] = t / nvf;
    }
    __syncthreads();
    for (int k = wave; k < m; k += 16) {
        float a = 0.f, b = 0.f;
        const float* r0row = X + rr0[k] * d;
        const float iv0 = inv[rr0[k]];
        for (int c = lane; c < d; c += 64) {
            a += P[(long long)k * d + c] * dP[(long long)k * d + c];
            b += (r0row[c] * iv0) * dcmv[c];
        }
        a = wave_reduce_sum(a); b = wave_reduce_sum(b);
        if (lane == 0) { dotP[k] = a; dot0[k] = b; }
    }
    __syncthreads();
    for (int c = tid; c < d; c += 1024) {
        for (int k = 0; k < m; ++k) {
            const long long r = rr[k];
            dE[r * d + c] += (dP[(long long)k * d + c] - P[(long long)k * d + c] * dotP[k]) * inv[r];
        }
        for (int k = 0; k < m; ++k) {
            if (!val[k]) continue;
            const long long r = rr0[k];
            const float iv = inv[r];
            dE[r * d + c] += (dcmv[c] - (X[r * d + c] * iv) * dot0[k]) * iv;
        }
    }
    if (wave == 15) {
        float a = 0.f, b = 0.f;
        for (int g = lane; g < G; g += 64) { a += dotpart[2 * g]; b += dotpart[2 * g + 1]; }
        a = wave_reduce_sum(a); b = wave_reduce_sum(b);
        if (lane == 0) { ddots[0] = a; ddots[1] = b; }
    }
}

bool pl_args_ok(const void* embds, const void* confs, const void* labs, int n, int d, int m, const void* proto0, const void* valid,
                const void* proto, const void* nearest, int use_max, int loss_mode, const void* workspace, long long workspace_floats) {
    if (!embds || !confs || !labs || !proto0 || !valid || !proto || !workspace || !pl_shape_ok(n, d, m)) return false;
    if (use_max && !nearest) return false;
    if (loss_mode < PL_SEPARATE || loss_mode > PL_NO_CONF) return false;
    return workspace_floats >= pl_plan(n, d, m).total;
}

}  // namespace

extern "C" long long effdet_episode_proj_loss_workspace_floats(int n, int d, int m) {
    if (!pl_shape_ok(n, d, m)) return -1;
    return pl_plan(n, d, m).total;
}

extern "C" int effdet_episode_proj_loss(void* stream, const float* embds, const float* confs, const long long* labs, int n, int d, int m,
                                        long long cls_id, const long long* cls_id_dev, float dot_mult, float dot_add, const float* dots,
                                        const long long* proto0, const unsigned char* valid, const long long* proto,
                                        const long long* nearest, int use_max, int loss_mode, float margin, float* workspace,
                                        long long workspace_floats, float* losses, float* inner_target, float* stats, int* counts) {
    EFFDET_ENTER();
    if (!losses || !inner_target || !stats || !counts ||
        !pl_args_ok(embds, confs, labs, n, d, m, proto0, valid, proto, nearest, use_max, loss_mode, workspace, workspace_floats))
        return EFFDET_EINVAL;
    const PlPlan p = pl_plan(n, d, m);
    const PlKept& k = p.kept;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* w = workspace;
    hipLaunchKernelGGL(pl_proto_kernel, dim3(1), dim3(1024), 0, st, embds, labs, n, d, m, cls_id, cls_id_dev, proto0, valid, proto, use_max,
                       loss_mode, margin, w + k.o_P, w + k.o_cmean, w + k.o_pmean, w + k.o_tc, w + k.o_nv, losses);
    hipLaunchKernelGGL(pl_rows_kernel, dim3(p.rows.G), dim3(256), 0, st, embds, confs, labs, n, d, m, p.rows.rows_per_block, cls_id, cls_id_dev,
                       dot_mult, dot_add, dots, nearest, use_max, loss_mode, margin, w + k.o_P, w + k.o_pmean, w + k.o_tc, w + k.o_inv,
                       w + k.o_s, w + k.o_sim, inner_target, w + p.o_fpart);
    hipLaunchKernelGGL(pl_final_kernel, dim3(1), dim3(64), 0, st, w + p.o_fpart, p.rows.G, n, losses, stats, counts);
    return effdet_check_launch();
}

extern "C" int effdet_episode_proj_loss_backward(void* stream, const float* embds, const float* confs, const long long* labs, int n, int d,
                                                 int m, long long cls_id, const long long* cls_id_dev, float dot_mult, float dot_add,
                                                 const float* dots, const long long* proto0, const unsigned char* valid,
                                                 const long long* proto, const long long* nearest, int use_max, int loss_mode,
                                                 float margin, const float* grad_losses, float* workspace, long long workspace_floats,
                                                 float* d_embds, float* d_confs, float* d_dots) {
    EFFDET_ENTER();
    if (!grad_losses || !d_embds || !d_confs || !d_dots ||
        !pl_args_ok(embds, confs, labs, n, d, m, proto0, valid, proto, nearest, use_max, loss_mode, workspace, workspace_floats))
        return EFFDET_EINVAL;
    const PlPlan p = pl_plan(n, d, m);
    const PlKept& k = p.kept;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float* w = workspace;
    hipLaunchKernelGGL(pl_bwd_rows_kernel, dim3(p.rows.G), dim3(256), 0, st, embds, confs, labs, n, d, m, p.rows.rows_per_block, cls_id,
                       cls_id_dev, dot_mult, dot_add, dots, nearest, use_max, loss_mode, margin, grad_losses, w + k.o_P, w + k.o_pmean,
                       w + k.o_tc, w + k.o_inv, w + k.o_s, w + k.o_sim, d_embds, d_confs, w + p.o_rowc, w + p.o_dotpart);
    hipLaunchKernelGGL((pl_part_kernel<false, float>), dim3(p.parts.parts, use_max ? m : 1), dim3(256), 0, st, embds, (const float*)nullptr,
                       nearest, n, d, m, p.parts.per, use_max, w + p.o_rowc, w + p.o_dPpart, (float*)nullptr, w + p.o_bTpart);
    hipLaunchKernelGGL(pl_bwd_proto_kernel, dim3(1), dim3(1024), 0, st, embds, labs, n, d, m, p.parts.parts, p.rows.G, cls_id, cls_id_dev,
                       proto0, valid, proto, use_max, loss_mode, margin, grad_losses, w + k.o_P, w + k.o_cmean, w + k.o_tc, w + k.o_nv,
                       w + k.o_inv, w + p.o_dPpart, w + p.o_bTpart, w + p.o_dotpart, w + p.o_dP, d_embds, d_dots);
    return effdet_check_launch();
}
