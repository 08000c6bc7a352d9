// The MAML inner update of the meta phase (infer.py:660-678) for a whole list of tensors at once:
//     forward    out_t[i] = p_t[i] - (lr[k_t] * g_t[i])                        one launch
//     backward   dg_t[i]  = -(lr[k_t] * G_t[i])                                 one launch, which also leaves per-workgroup partials of
//                dlr_k    = -sum_{t: k_t = k} sum_i G_t[i] * g_t[i]             G g; a second launch adds them up per step size
// (dp_t is G_t itself and needs no kernel.)  This unit is compiled with -ffp-contract=off: the product and the difference round
// separately, so the results carry the bits of torch's `par - par_lr * inner_grad` and of its autograd gradient `(-G) * lr`.
//
// Every tensor is cut into PIECES of at most PIECE floats; a workgroup owns one piece, so its tensor, and with it the step size,
// is wave-uniform.  Pointers, counts, the piece ranges and the step-size table travel by value in the kernel arguments: nothing is
// uploaded, nothing is read back, and a captured launch stays valid.  A step size is read through its device pointer when it has
// one, so a value changed in place is seen by the next launch (or graph replay).  16-byte accesses are used for a tensor only when
// all three of its pointers are 16-byte aligned; a view at an odd 4-byte offset, or a 9-element tensor's tail, takes the scalar path.
//
// dlr is accumulated in float64 from the float32 inputs (every product G g is exact in float64): per lane in index order, then a
// fixed tree over the workgroup, then - second launch - a fixed strided pass and tree over the partials of the tensors that share
// the step size, with ONE rounding to float32 at the end.  No atomics: two calls give the same bits.
#include "common.h"

namespace {

constexpr int MAX_TENSORS = 32;
constexpr int MAX_LR = 16;
constexpr int PIECE = 2048;                       // floats per workgroup: 256 lanes x 2 x 16 bytes
constexpr long long MAX_COUNT = 1ll << 30;        // elements per tensor (piece offsets and the piece total stay in int)

struct Args {
    const float* a[MAX_TENSORS];                  // p (forward) / G (backward)
    const float* g[MAX_TENSORS];
    float* o[MAX_TENSORS];                        // out (forward) / dg (backward, NULL: not wanted)
    const float* lr_ptr[MAX_LR];                  // device pointer of step size k, or NULL: lr_val[k]
    float lr_val[MAX_LR];
    int count[MAX_TENSORS];
    int piece_start[MAX_TENSORS + 1];             // tensor t owns the workgroups [piece_start[t], piece_start[t + 1])
    int lr_index[MAX_TENSORS];
    int n;
};

struct Piece { const float* a; const float* g; float* o; float lr; int len; bool vec; };

DEV Piece find_piece(const Args& s) {
    const int b = blockIdx.x;
    int t = 0;
    while (t + 1 < s.n && b >= s.piece_start[t + 1]) ++t;
    const int base = (b - s.piece_start[t]) * PIECE;
    const int rest = s.count[t] - base;
    const int k = s.lr_index[t];
    const float* lp = s.lr_ptr[k];
    Piece pc;
    pc.a = s.a[t] + base;
    pc.g = s.g[t] + base;
    pc.o = s.o[t] ? s.o[t] + base : nullptr;
    pc.lr = lp ? *lp : s.lr_val[k];
    pc.len = rest < PIECE ? rest : PIECE;
    pc.vec = ((reinterpret_cast<uintptr_t>(pc.a) | reinterpret_cast<uintptr_t>(pc.g) | reinterpret_cast<uintptr_t>(pc.o)) & 15) == 0;
    return pc;
}

__global__ __launch_bounds__(256) void inner_update_kernel(Args s) {
    const Piece pc = find_piece(s);
    const int tid = threadIdx.x;
    int done = 0;
    if (pc.vec) {
        const int nv = pc.len >> 2;
        const f32x4* a4 = reinterpret_cast<const f32x4*>(pc.a);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(pc.g);
        f32x4* o4 = reinterpret_cast<f32x4*>(pc.o);
        f32x4 av[2], gv[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * 256;
            if (i < nv) { av[k] = a4[i]; gv[k] = g4[i]; }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * 256;
            if (i < nv) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = av[k][e] - pc.lr * gv[k][e];
                o4[i] = r;
            }
        }
        done = nv << 2;
    }
    for (int i = done + tid; i < pc.len; i += 256) pc.o[i] = pc.a[i] - pc.lr * pc.g[i];
}

// the 256 lanes' doubles, added in a fixed tree
DEV double block_sum_f64(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// SUM: also partial[workgroup] = sum over the piece of G g
template <bool SUM>
__global__ __launch_bounds__(256) void inner_update_bwd_kernel(Args s, double* __restrict__ partial) {
    __shared__ double red[256];
    const Piece pc = find_piece(s);
    const int tid = threadIdx.x;
    double acc = 0.0;
    int done = 0;
    if (pc.vec) {
        const int nv = pc.len >> 2;
        const f32x4* a4 = reinterpret_cast<const f32x4*>(pc.a);
        const f32x4* g4 = reinterpret_cast<const f32x4*>(pc.g);
        f32x4* o4 = reinterpret_cast<f32x4*>(pc.o);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * 256;
            if (i < nv) {
                const f32x4 G = a4[i];
                if (o4) {
                    f32x4 r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[e] = -(pc.lr * G[e]);
                    o4[i] = r;
                }
                if (SUM) {
                    const f32x4 g = g4[i];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc += (double)G[e] * (double)g[e];
                }
            }
        }
        done = nv << 2;
    }
    for (int i = done + tid; i < pc.len; i += 256) {
        const float G = pc.a[i];
        if (pc.o) pc.o[i] = -(pc.lr * G);
        if (SUM) acc += (double)G * (double)pc.g[i];
    }
    if (SUM) {
        acc = block_sum_f64(acc, red);
        if (tid == 0) partial[blockIdx.x] = acc;
    }
}

// one workgroup per step size k: total[k] = (accumulate ? total[k] : 0) + the partials of the tensors with k_t = k, in a fixed
// order; dlr[k] = float(-total[k])
__global__ __launch_bounds__(256) void inner_update_lr_kernel(Args s, const double* __restrict__ partial, int accumulate,
                                                              double* __restrict__ total, float* __restrict__ dlr) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (int t = 0; t < s.n; ++t) {
        if (s.lr_index[t] != k) continue;
        for (int i = s.piece_start[t] + tid; i < s.piece_start[t + 1]; i += 256) acc += partial[i];
    }
    acc = block_sum_f64(acc, red);
    if (tid == 0) {
        const double tot = accumulate ? total[k] + acc : acc;
        total[k] = tot;
        dlr[k] = (float)(-tot);
    }
}

// validates and fills the by-value argument block; the number of pieces (workgroups), or EFFDET_EINVAL
long long fill_args(Args& s, int n, const void* const* a, const void* const* g, void* const* o, bool need_o, const long long* count,
                    const int* lr_index, int n_lr, const void* const* lr_ptr, const float* lr_val) {
    if (!a || !g || !o || !count || !lr_index || !lr_ptr || !lr_val) return EFFDET_EINVAL;
    if (n < 1 || n > MAX_TENSORS || n_lr < 1 || n_lr > MAX_LR) return EFFDET_EINVAL;
    s = Args{};
    long long pieces = 0;
    for (int t = 0; t < n; ++t) {
        if (!a[t] || !g[t] || (need_o && !o[t])) return EFFDET_EINVAL;
        if (count[t] < 1 || count[t] > MAX_COUNT) return EFFDET_EINVAL;
        if (lr_index[t] < 0 || lr_index[t] >= n_lr) return EFFDET_EINVAL;
        s.a[t] = static_cast<const float*>(a[t]);
        s.g[t] = static_cast<const float*>(g[t]);
        s.o[t] = static_cast<float*>(o[t]);
        s.count[t] = (int)count[t];
        s.lr_index[t] = lr_index[t];
        s.piece_start[t] = (int)pieces;
        pieces += (count[t] + PIECE - 1) / PIECE;
    }
    s.piece_start[n] = (int)pieces;
    for (int k = 0; k < n_lr; ++k) {
        s.lr_ptr[k] = static_cast<const float*>(lr_ptr[k]);
        s.lr_val[k] = lr_val[k];
    }
    s.n = n;
    return pieces;
}

}  // namespace

extern "C" int effdet_inner_update_max_tensors(void) { return MAX_TENSORS; }
extern "C" int effdet_inner_update_max_step_sizes(void) { return MAX_LR; }

extern "C" long long effdet_inner_update_workspace_doubles(int n_tensors, const long long* count) {
    if (!count || n_tensors < 1 || n_tensors > MAX_TENSORS) return -1;
    long long pieces = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (count[t] < 1 || count[t] > MAX_COUNT) return -1;
        pieces += (count[t] + PIECE - 1) / PIECE;
    }
    return MAX_LR + pieces;
}

extern "C" int effdet_inner_update(void* stream, int n_tensors, const void* const* p, const void* const* g, void* const* out,
                                   const long long* count, const int* lr_index, int n_lr, const void* const* lr_ptr,
                                   const float* lr_val) {
    EFFDET_ENTER();
    Args s;
    const long long pieces = fill_args(s, n_tensors, p, g, out, true, count, lr_index, n_lr, lr_ptr, lr_val);
    if (pieces < 0) return EFFDET_EINVAL;
    hipLaunchKernelGGL(inner_update_kernel, dim3((unsigned)pieces), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), s);
    return effdet_check_launch();
}

extern "C" int effdet_inner_update_backward(void* stream, int n_tensors, const void* const* grad_out, const void* const* g,
                                            void* const* dg, const long long* count, const int* lr_index, int n_lr,
                                            const void* const* lr_ptr, const float* lr_val, double* workspace,
                                            long long workspace_doubles, int accumulate, float* dlr) {
    EFFDET_ENTER();
    Args s;
    const long long pieces = fill_args(s, n_tensors, grad_out, g, dg, false, count, lr_index, n_lr, lr_ptr, lr_val);
    if (pieces < 0) return EFFDET_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!dlr) {
        bool any = false;
        for (int t = 0; t < n_tensors; ++t) any = any || dg[t] != nullptr;
        if (any) hipLaunchKernelGGL(inner_update_bwd_kernel<false>, dim3((unsigned)pieces), dim3(256), 0, st, s, nullptr);
        return effdet_check_launch();
    }
    if (!workspace || workspace_doubles < MAX_LR + pieces || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return EFFDET_EINVAL;
    double* partial = workspace + MAX_LR;
    hipLaunchKernelGGL(inner_update_bwd_kernel<true>, dim3((unsigned)pieces), dim3(256), 0, st, s, partial);
    hipLaunchKernelGGL(inner_update_lr_kernel, dim3((unsigned)n_lr), dim3(256), 0, st, s, partial, accumulate ? 1 : 0, workspace, dlr);
    return effdet_check_launch();
}
