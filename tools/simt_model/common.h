// A CPU model of the SIMT execution, enough to run csrc/episode_loss.hip and csrc/episode_support.hip as host C++ (tools/simt_model/run.py copies the kernel
// source beside this file, where `#include "common.h"` finds it instead of csrc/common.h): one std::thread per thread of a
// workgroup, the workgroups one after another, a barrier for __syncthreads and one per wave for the shuffles and the ballot.
// __shared__ is a function-local static, shared by the threads of the one workgroup that is running.  It checks the arithmetic and
// the indexing of a kernel, not its timing or its memory model.
#pragma once
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>
#include <barrier>
#include <memory>
#include <algorithm>
#define DEV static inline
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define EFFDET_ENTER() (void)0
#define EFFDET_OK 0
#define EFFDET_EINVAL 1
#define EFFDET_ELAUNCH 2
static inline int effdet_check_launch() { return 0; }
typedef void* hipStream_t;
struct dim3 { int x, y, z; dim3(int a = 1, int b = 1, int c = 1) : x(a), y(b), z(c) {} };
struct SimCtx { std::barrier<>* block; std::barrier<>* wave; double* xf; int* xi; float* xm; };
static thread_local dim3 threadIdx, blockIdx, gridDim;
static thread_local SimCtx simctx;
static inline void __syncthreads() { simctx.block->arrive_and_wait(); }
static inline int __builtin_amdgcn_readfirstlane(int v) { return v; }
template <class T> static inline T __shfl_xor(T v, int o, int) {
    const int lane = threadIdx.x & 63;
    simctx.xf[lane] = v; simctx.wave->arrive_and_wait();
    const T r = (T)simctx.xf[lane ^ o]; simctx.wave->arrive_and_wait();
    return r;
}
// The shuffles pass values through a double: exact for float, double and 32-bit integers, not for 64-bit ones.
template <class T> static inline T __shfl_up(T v, int o, int) {
    const int lane = threadIdx.x & 63;
    simctx.xf[lane] = (double)v; simctx.wave->arrive_and_wait();
    const T r = lane >= o ? (T)simctx.xf[lane - o] : v; simctx.wave->arrive_and_wait();
    return r;
}
template <class T> static inline T __shfl_down(T v, int o, int) {
    const int lane = threadIdx.x & 63;
    simctx.xf[lane] = (double)v; simctx.wave->arrive_and_wait();
    const T r = lane + o < 64 ? (T)simctx.xf[lane + o] : v; simctx.wave->arrive_and_wait();
    return r;
}
static inline unsigned long long __ballot(bool p) {
    const int lane = threadIdx.x & 63;
    simctx.xi[lane] = p ? 1 : 0; simctx.wave->arrive_and_wait();
    unsigned long long r = 0;
    for (int i = 0; i < 64; ++i) if (simctx.xi[i]) r |= 1ull << i;
    simctx.wave->arrive_and_wait();
    return r;
}
// integer atomics (csrc/ood_eval.hip: LDS digit counts, flag bits) and a barrier for the lanes of one wave
template <class T> static inline T atomicAdd(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class T> static inline T atomicOr(T* p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline void sim_wave_sync() { simctx.wave->arrive_and_wait(); }
static inline void __builtin_amdgcn_wave_barrier() { sim_wave_sync(); }
DEV float wave_reduce_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
DEV float wave_reduce_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64)); return v; }
static inline float __int_as_float(int v) { float f; std::memcpy(&f, &v, 4); return f; }
static inline int __float_as_int(float f) { int v; std::memcpy(&v, &f, 4); return v; }
static inline unsigned __float_as_uint(float f) { unsigned v; std::memcpy(&v, &f, 4); return v; }
// the high word of a 32 x 32 -> 64 bit product (csrc/outlier_synth.hip: Philox4x32)
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
template <class K, class... A>
void sim_launch(K kernel, dim3 grid, dim3 block, A... args) {
    const int nt = block.x, nw = (nt + 63) / 64;
    for (int by = 0; by < grid.y; ++by)
        for (int bx = 0; bx < grid.x; ++bx) {
            std::barrier<> bb(nt);
            std::vector<std::unique_ptr<std::barrier<>>> wb;
            std::vector<std::vector<double>> xf(nw, std::vector<double>(64));
            std::vector<std::vector<int>> xi(nw, std::vector<int>(64));
            std::vector<std::vector<float>> xm(nw, std::vector<float>(64 * 8));
            for (int w = 0; w < nw; ++w) wb.emplace_back(new std::barrier<>(std::min(64, nt - 64 * w)));
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t)
                th.emplace_back([&, t] {
                    threadIdx = dim3(t); blockIdx = dim3(bx, by); gridDim = grid;
                    simctx = SimCtx{&bb, wb[t / 64].get(), xf[t / 64].data(), xi[t / 64].data(), xm[t / 64].data()};
                    kernel(args...);
                });
            for (auto& x : th) x.join();
        }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) sim_launch(k, g, b, __VA_ARGS__)
using std::fmax; using std::sqrt; using std::exp;
// The float32-input MFMA of csrc/common.h's mma_chunk (csrc/feature_ood.hip): four v_mfma_f32_16x16x4_f32 on a 64-byte K-chunk.
// Lane l supplies row / column (l & 15) and K values 4 * (l >> 4) + s, s = 0 .. 3, of both operands; instruction s multiplies the
// K values {s, 4 + s, 8 + s, 12 + s}, an fmaf chain in that order (exact float32); C/D: column l & 15, row 4 * (l >> 4) + reg.
typedef float f32x4 __attribute__((vector_size(16)));
static inline float __uint_as_float(unsigned v) { float f; std::memcpy(&f, &v, 4); return f; }
template <typename T> struct Frag;
template <> struct Frag<float> { f32x4 v; };
template <typename T> static inline Frag<T> ld_frag(const void* p) { Frag<T> f; std::memcpy(&f.v, p, sizeof(f.v)); return f; }
static inline void mma_chunk(const Frag<float>& a, const Frag<float>& b, f32x4& acc) {
    const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    for (int s = 0; s < 4; ++s) { simctx.xm[lane * 8 + s] = a.v[s]; simctx.xm[lane * 8 + 4 + s] = b.v[s]; }
    simctx.wave->arrive_and_wait();
    for (int s = 0; s < 4; ++s)
        for (int kg = 0; kg < 4; ++kg)
            for (int r = 0; r < 4; ++r)
                acc[r] = std::fmaf(simctx.xm[(16 * kg + 4 * g + r) * 8 + s], simctx.xm[(16 * kg + col) * 8 + 4 + s], acc[r]);
    simctx.wave->arrive_and_wait();
}
