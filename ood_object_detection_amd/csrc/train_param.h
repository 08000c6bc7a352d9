// The parameter-sized formulas of the float32 training path, each stated once: the BN(eval) fold, the nn.BatchNorm2d bookkeeping,
// the BN backward vectors, the BiFPN edge weights and the closed-form conv + BN parameter gradients, with the two op records the
// stage tables are made of.  Callers: train_net.hip (single ops, stage tables, the flat BatchNorm second stages) and
// train_levels.hip (the per-level BatchNorm second stages).  Both units are built with -ffp-contract=off, so one text gives the
// same bits wherever it is used.
#pragma once
#include "common.h"

namespace {

// rstd = 1/sqrt(var + eps), scale = gamma * rstd, shift = beta - mean * scale of one channel
struct BnAffine { float rstd, scale, shift; };
DEV BnAffine bn_affine(float gamma, float beta, float mean, float var, float eps) {
    BnAffine r;
    r.rstd = 1.0f / sqrtf(var + eps);
    r.scale = gamma * r.rstd;
    r.shift = beta - mean * r.scale;
    return r;
}

// nn.BatchNorm2d running statistics of one channel in training mode: r = (1 - momentum) r + momentum * batch, unbiased variance
DEV void bn_track(float* running_mean, float* running_var, float mean, float var, float momentum, float unbias) {
    *running_mean = *running_mean * (1.0f - momentum) + momentum * mean;
    *running_var = *running_var * (1.0f - momentum) + momentum * (var * unbias);
}

// BN backward of one channel from s1 = sum(dy), s2 = sum(dy (c - mean)): d gamma, d beta, and v1 = s1 / M, v3 = rstd^2 s2 / M for
// op 6 of the element-wise family
DEV void bn_bwd_vectors(float s1, float s2, float rstd, float invM, float* dgamma, float* dbeta, float* v1, float* v3) {
    *dgamma = s2 * rstd;
    *dbeta = s1;
    *v1 = s1 * invM;
    *v3 = rstd * rstd * s2 * invM;
}

// BiFPN edge weights of a node with n inputs -> wdev = {w0, w1, w2, den}.  method 0 'fastattn': relu, den = sum + 1e-4;
// 1 'attn': softmax, den = 1; 2 'sum': ones, den = 1 (ewp is not read)
DEV void fpn_edge_weights(const float* ewp, int n, int method, float* wdev) {
    float w[3] = {0.f, 0.f, 0.f};
    float den = 1.0f;
    if (method == 0) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) { w[i] = fmaxf(ewp[i], 0.f); s += w[i]; }
        den = s + 0.0001f;
    } else if (method == 1) {
        float m = ewp[0];
        for (int i = 1; i < n; ++i) m = fmaxf(m, ewp[i]);
        float s = 0.f;
        for (int i = 0; i < n; ++i) { w[i] = expf(ewp[i] - m); s += w[i]; }
        for (int i = 0; i < n; ++i) w[i] = w[i] / s;
    } else {
        for (int i = 0; i < n; ++i) w[i] = 1.0f;
    }
    wdev[0] = w[0]; wdev[1] = w[1]; wdev[2] = w[2]; wdev[3] = den;
}

// One record of a stage's prep table (mirrored by train_engine._PrepOp), also what a single op hands its kernel by value.
//   kind 0: dst0 [cols][rows] = src [rows][cols] transposed
//   kind 1: BN(eval) fold of W = src [N = rows][K = cols]: dst0 = Wf = W * scale[n], dst1 = WfT [K][N], dst2 = WT [K][N] (each optional)
//   kind 2: fpn_edge_weights(src, rows, (int)eps) -> dst0 (cols = 1)
struct PrepOp {
    int kind, rows, cols; float eps;
    const float* src; const float* gamma; const float* beta; const float* mean; const float* var;
    float* dst0; float* dst1; float* dst2; float* scale; float* shift; float* rstd;
};
static_assert(sizeof(PrepOp) == 104, "train_engine._PrepOp mirrors this layout");

// the workgroups of grid row x stride over the elements of one op (nothing is reduced: the bits do not depend on the grid)
DEV void prep_op_run(const PrepOp& p) {
    if (p.kind == 2) {
        if (blockIdx.x == 0 && threadIdx.x == 0) fpn_edge_weights(p.src, p.rows, (int)p.eps, p.dst0);
        return;
    }
    const long long total = (long long)p.rows * p.cols;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int r = (int)(e / p.cols), c = (int)(e - (long long)r * p.cols);
        const long long eT = (long long)c * p.rows + r;
        const float w = p.src[e];
        if (p.kind == 0) { p.dst0[eT] = w; continue; }
        const BnAffine a = bn_affine(p.gamma[r], p.beta[r], p.mean[r], p.var[r], p.eps);
        if (c == 0) { p.scale[r] = a.scale; p.shift[r] = a.shift; p.rstd[r] = a.rstd; }
        if (p.dst0) p.dst0[e] = w * a.scale;
        if (p.dst1) p.dst1[eT] = w * a.scale;
        if (p.dst2) p.dst2[eT] = w;
    }
}

// One record of a stage's gradient table (mirrored by train_engine._GradOp).  z = scale * conv(x; W) + shift, dWraw = dz^T x,
// dsum = sum dz  ->  dW = scale * dWraw, d gamma = rstd * (sum_k W * dWraw - mean * dsum), d beta = dsum.
// dWext: [N][K] then [N] sums, or [(K + 1)][N] when transposed: both layouts keep the N sums behind the N * K gradients.
struct GradOp {
    const float* dWext; const float* W; const float* scale; const float* rstd; const float* mean;
    float* dW; float* dgamma; float* dbeta; int N, K, transposed, pad;
};
static_assert(sizeof(GradOp) == 80, "train_engine._GradOp mirrors this layout");

// one workgroup of 256 threads per output channel n = blockIdx.x (the workgroups past a short row of a table return at once)
DEV void grad_op_run(const GradOp& p) {
    __shared__ float sm[4];
    const int n = blockIdx.x;
    if (n >= p.N) return;                        // uniform per workgroup
    const float sc = p.scale[n];
    float acc = 0.f;
    for (int k = threadIdx.x; k < p.K; k += 256) {
        const float v = p.transposed ? p.dWext[(long long)k * p.N + n] : p.dWext[(long long)n * p.K + k];
        p.dW[(long long)n * p.K + k] = sc * v;
        acc += p.W[(long long)n * p.K + k] * v;
    }
    acc = wave_reduce_sum(acc);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tot = ((sm[0] + sm[1]) + sm[2]) + sm[3];
        const float dsum = p.dWext[(long long)p.K * p.N + n];
        p.dgamma[n] = p.rstd[n] * (tot - p.mean[n] * dsum);
        p.dbeta[n] = dsum;
    }
}

}  // namespace
