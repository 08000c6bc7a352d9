// Grouped optimizer: torch.nn.utils.clip_grad_norm_ per clip domain followed by torch.optim.Adam / torch.optim.SGD with
// parameter groups (pretrain.py:179-187, :279-281; infer.py:259-286, :803-804) on flat float32 buffers, in three launches.
//
// Every parameter tensor is a SEGMENT of the flat buffers (start and padded length multiples of 16 floats, padding zero).  A
// segment is cut into PIECES of at most GROUP_PIECE floats that never straddle segments; a workgroup owns one piece, so what it
// needs to know about its segment (clip coefficient, step size, hyper-parameters of the group) is wave-uniform and fetched once.
// The planner (optim.plan_layout) puts the segments of one clip domain next to each other: a domain is one range of pieces.
//
//   1. group_sqnorm_kernel   one partial sum of squares per piece of a domain (0 for a segment that is not present)
//   2. group_finish_kernel   one workgroup per domain (+ one for the segments in no domain): adds the partials in a fixed order,
//                            forms the clip coefficient, and for every segment of the domain advances the step count and writes
//                            the segment's constants {step size, 1/sqrt(bc2), coef, flags}
//   3. group_update_kernel   one pass over p, g and the state with 16-byte accesses
// No atomics, fixed-order sums (two runs give the same bits), nothing read back.  Learning rates, max norms, present flags live in
// device memory (`dyn`), the step counts are advanced by kernel 2: one captured launch sequence serves every later step.
#include "common.h"

namespace {

constexpr int GROUP_PIECE = 2048;                 // floats per piece: 256 lanes x 2 x 16 bytes
constexpr int PIECE_VEC = GROUP_PIECE / 4;
constexpr int GROUP_ROW = 16;                     // 4-byte words per group row of `dyn`

// group row of `dyn`, as written by optim.GroupedOptimizer._host_words
struct GroupRow {
    double lr, beta1, beta2;                      // words 0-5 (doubles: torch forms lr / bc1 and the bias corrections in double)
    float wd, eps, omb1, b2, omb2, momentum;      // words 6-11: float(1 - beta1), float(beta2), float(1 - beta2)
    int nesterov;                                 // word 12
    int pad[3];
};
static_assert(sizeof(GroupRow) == GROUP_ROW * 4, "group row layout");

struct Tables {
    const int* pieces;        // [n_pieces][4]   {offset in 16-byte units, 16-byte units, segment, 0}
    const int* seg_group;     // [n_seg]         group of the segment, -1: in no group (norm only)
    const int* dom_ranges;    // [n_dom + 1][4]  {first piece, end piece, first segment, end segment}; last row: segments in no domain
    const int* dyn;           // [n_groups] group rows, then max_norm[n_dom] (float), then present[n_seg] (int)
    int n_pieces, n_norm_pieces, n_seg, n_dom, n_groups;
    long long n_vec;          // 16-byte units in each flat buffer
};

DEV const GroupRow* group_row(const Tables& t, int g) { return reinterpret_cast<const GroupRow*>(t.dyn) + g; }
DEV float dom_max_norm(const Tables& t, int d) { return __builtin_bit_cast(float, t.dyn[t.n_groups * GROUP_ROW + d]); }
DEV int seg_present(const Tables& t, int s) { return t.dyn[t.n_groups * GROUP_ROW + t.n_dom + s]; }

// a piece whose table entry does not fit the buffers is skipped (never dereferenced)
DEV bool piece_ok(const Tables& t, int4 pc) {
    return pc.x >= 0 && pc.y > 0 && pc.y <= PIECE_VEC && (long long)pc.x + pc.y <= t.n_vec && pc.z >= 0 && pc.z < t.n_seg;
}

DEV float block_sum_256(float s, float* part) {
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void group_sqnorm_kernel(Tables t, const f32x4* __restrict__ g, float* __restrict__ partial) {
    __shared__ float part[4];
    const int4 pc = reinterpret_cast<const int4*>(t.pieces)[blockIdx.x];
    float s = 0.f;
    if (piece_ok(t, pc) && seg_present(t, pc.z)) {
        const f32x4* gp = g + pc.x;
        f32x4 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = threadIdx.x + k * 256;
            v[k] = i < pc.y ? gp[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) s += (v[k][0] * v[k][0] + v[k][1] * v[k][1]) + (v[k][2] * v[k][2] + v[k][3] * v[k][3]);
    }
    s = block_sum_256(s, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// b^t for t >= 1 by squaring, in double (the bias corrections 1 - beta^t of torch are Python doubles)
DEV double pow_int(double b, int t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// kind 0: Adam, 1: SGD.  advance 0: norms only (grad_norm()).
__global__ __launch_bounds__(256) void group_finish_kernel(Tables t, int kind, int advance, const float* __restrict__ partial,
                                                           float* __restrict__ norms, int* __restrict__ step, int4* __restrict__ seg_const) {
    __shared__ float part[4];
    const int d = blockIdx.x;
    const int4 r = reinterpret_cast<const int4*>(t.dom_ranges)[d];
    float coef = 1.f;
    if (d < t.n_dom) {
        float s = 0.f;
        for (int i = r.x + (int)threadIdx.x; i < r.y; i += 256) s += partial[i];
        s = block_sum_256(s, part);
        const float norm = sqrtf(s);
        if (threadIdx.x == 0) norms[d] = norm;
        coef = dom_max_norm(t, d) / (norm + 1e-6f);                 // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
        coef = coef > 1.f ? 1.f : coef;
    }
    if (!advance) return;
    for (int s = r.z + (int)threadIdx.x; s < r.w; s += 256) {
        const int g = t.seg_group[s];
        const bool active = g >= 0 && g < t.n_groups && seg_present(t, s) != 0;
        float step_size = 0.f, inv_bc2s = 0.f;
        int flags = 0;
        if (active) {
            const GroupRow* gr = group_row(t, g);
            const int before = step[s];
            flags = 1;
            if (kind == 0) {
                const int n = before + 1;
                step[s] = n;
                const double bc1 = 1.0 - pow_int(gr->beta1, n), bc2 = 1.0 - pow_int(gr->beta2, n);
                step_size = (float)(gr->lr / bc1);
                inv_bc2s = (float)(1.0 / sqrt(bc2));
            } else {
                step_size = (float)gr->lr;
                if (gr->momentum != 0.f) {                          // torch creates the buffer at the first update with momentum
                    if (before == 0) flags |= 2;
                    step[s] = 1;
                }
            }
        }
        // Four 32-bit words per segment.  The floats are bit-cast from plain float variables: __builtin_bit_cast applied to an
        // element of an ext_vector_type (`c[3]`) reads the vector's first element, whichever index is named.
        int4 w;
        w.x = __builtin_bit_cast(int, step_size);
        w.y = __builtin_bit_cast(int, inv_bc2s);
        w.z = __builtin_bit_cast(int, coef);
        w.w = flags;
        seg_const[s] = w;
    }
}

// torch/optim/adam.py::_single_tensor_adam: g += wd p; m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, 1 - b2);
// denom = sqrt(v) / sqrt(bc2) + eps; p.addcdiv_(m, denom, -lr / bc1)
DEV void adam4(f32x4& p, f32x4 g, f32x4& m, f32x4& v, const GroupRow& gr, float coef, float step_size, float inv_bc2s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float ge = g[e] * coef;
        if (gr.wd != 0.f) ge = ge + gr.wd * p[e];
        const float me = m[e] + gr.omb1 * (ge - m[e]);
        const float ve = v[e] * gr.b2 + (gr.omb2 * ge) * ge;
        const float denom = sqrtf(ve) * inv_bc2s + gr.eps;
        p[e] = p[e] - (step_size * me) / denom;
        m[e] = me;
        v[e] = ve;
    }
}

// torch/optim/sgd.py::_single_tensor_sgd, dampening 0
DEV void sgd4(f32x4& p, f32x4 g, f32x4& buf, const GroupRow& gr, float coef, float lr, bool first) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float ge = g[e] * coef;
        if (gr.wd != 0.f) ge = ge + gr.wd * p[e];
        if (gr.momentum != 0.f) {
            const float be = first ? ge : buf[e] * gr.momentum + ge;
            buf[e] = be;
            ge = gr.nesterov ? ge + gr.momentum * be : be;
        }
        p[e] = p[e] - lr * ge;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void group_update_kernel(Tables t, const int4* __restrict__ seg_const, f32x4* __restrict__ p,
                                                           const f32x4* __restrict__ g, f32x4* __restrict__ s1, f32x4* __restrict__ s2) {
    const int4 pc = reinterpret_cast<const int4*>(t.pieces)[blockIdx.x];
    if (!piece_ok(t, pc)) return;
    const int4 ci = seg_const[pc.z];
    const int flags = ci.w, w0 = ci.x, w1 = ci.y, w2 = ci.z;
    const float step_size = __builtin_bit_cast(float, w0), inv_bc2s = __builtin_bit_cast(float, w1), coef = __builtin_bit_cast(float, w2);
    if (!(flags & 1)) return;                                       // not present, or in no group: no byte of it is touched
    const GroupRow gr = *group_row(t, t.seg_group[pc.z]);
    const bool use_buf = KIND == 0 || gr.momentum != 0.f;
    const bool read_buf = KIND == 0 || (use_buf && !(flags & 2));
    const long long base = pc.x;
    f32x4 pv[2], gv[2], av[2], bv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < pc.y) {
            pv[k] = p[base + i];
            gv[k] = g[base + i];
            av[k] = read_buf ? s1[base + i] : f32x4{0.f, 0.f, 0.f, 0.f};
            if (KIND == 0) bv[k] = s2[base + i];
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < pc.y) {
            if (KIND == 0) {
                adam4(pv[k], gv[k], av[k], bv[k], gr, coef, step_size, inv_bc2s);
                s2[base + i] = bv[k];
            } else {
                sgd4(pv[k], gv[k], av[k], gr, coef, step_size, (flags & 2) != 0);
            }
            if (use_buf) s1[base + i] = av[k];
            p[base + i] = pv[k];
        }
    }
}

int fill_tables(Tables& t, const int* pieces, int n_pieces, int n_norm_pieces, const int* seg_group, int n_seg, const int* dom_ranges,
                int n_dom, const int* dyn, int n_groups, long long n_floats) {
    if (!pieces || !seg_group || !dom_ranges || !dyn) return EFFDET_EINVAL;
    if (n_pieces <= 0 || n_norm_pieces < 0 || n_norm_pieces > n_pieces || n_seg <= 0 || n_dom < 0 || n_groups < 0) return EFFDET_EINVAL;
    if (n_floats <= 0 || (n_floats & 15) != 0) return EFFDET_EINVAL;
    t = Tables{pieces, seg_group, dom_ranges, dyn, n_pieces, n_norm_pieces, n_seg, n_dom, n_groups, n_floats / 4};
    return EFFDET_OK;
}

void launch_norms(hipStream_t st, const Tables& t, int kind, int advance, const float* grad, float* partial, float* norms, int* step,
                  float* seg_const) {
    if (t.n_norm_pieces > 0)
        hipLaunchKernelGGL(group_sqnorm_kernel, dim3((unsigned)t.n_norm_pieces), dim3(256), 0, st, t, reinterpret_cast<const f32x4*>(grad), partial);
    hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)(t.n_dom + (advance ? 1 : 0))), dim3(256), 0, st, t, kind, advance, partial, norms,
                       step, reinterpret_cast<int4*>(seg_const));
}

}  // namespace

extern "C" long long effdet_group_piece_floats(void) { return GROUP_PIECE; }

extern "C" int effdet_group_norms(void* stream, const float* grad, long long n_floats, const int* pieces, int n_pieces, int n_norm_pieces,
                                  const int* seg_group, int n_segments, const int* dom_ranges, int n_domains, const int* dyn,
                                  int n_groups, float* partial, float* norms) {
    EFFDET_ENTER();
    Tables t;
    if (!grad || !partial || !norms || n_domains <= 0) return EFFDET_EINVAL;
    if (fill_tables(t, pieces, n_pieces, n_norm_pieces, seg_group, n_segments, dom_ranges, n_domains, dyn, n_groups, n_floats) != EFFDET_OK)
        return EFFDET_EINVAL;
    launch_norms(reinterpret_cast<hipStream_t>(stream), t, 0, 0, grad, partial, norms, nullptr, nullptr);
    return effdet_check_launch();
}

extern "C" int effdet_group_step(void* stream, int kind, float* param, const float* grad, float* state1, float* state2, long long n_floats,
                                 const int* pieces, int n_pieces, int n_norm_pieces, const int* seg_group, int n_segments,
                                 const int* dom_ranges, int n_domains, const int* dyn, int n_groups, int* step, float* seg_const,
                                 float* partial, float* norms) {
    EFFDET_ENTER();
    Tables t;
    if (!param || !grad || !state1 || (kind == 0 && !state2) || !step || !seg_const || !partial || !norms) return EFFDET_EINVAL;
    if ((kind != 0 && kind != 1) || n_groups <= 0) return EFFDET_EINVAL;
    if (fill_tables(t, pieces, n_pieces, n_norm_pieces, seg_group, n_segments, dom_ranges, n_domains, dyn, n_groups, n_floats) != EFFDET_OK)
        return EFFDET_EINVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    launch_norms(st, t, kind, 1, grad, partial, norms, step, seg_const);
    if (kind == 0)
        hipLaunchKernelGGL(group_update_kernel<0>, dim3((unsigned)n_pieces), dim3(256), 0, st, t, reinterpret_cast<const int4*>(seg_const),
                           reinterpret_cast<f32x4*>(param), reinterpret_cast<const f32x4*>(grad), reinterpret_cast<f32x4*>(state1),
                           reinterpret_cast<f32x4*>(state2));
    else
        hipLaunchKernelGGL(group_update_kernel<1>, dim3((unsigned)n_pieces), dim3(256), 0, st, t, reinterpret_cast<const int4*>(seg_const),
                           reinterpret_cast<f32x4*>(param), reinterpret_cast<const f32x4*>(grad), reinterpret_cast<f32x4*>(state1),
                           reinterpret_cast<f32x4*>(state2));
    return effdet_check_launch();
}
