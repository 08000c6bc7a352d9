// The rows x d x C product of csrc/vmf.hip's logits, l[i][c] = logZ_c + kappa_c (mu_c . r_i), in its two forms on the same data:
//   valu   the form vmf.hip ships: a wave per row, r in the wave's LDS, lane t owns classes t, t + 64 and walks d over mu^T [d][C]
//   mfma   the float32-input MFMA (v_mfma_f32_16x16x4_f32, four per 16-wide K chunk as common.h's mma_chunk): a wave takes 16 rows,
//          lane l supplies row l & 15 and the K piece 4 (l >> 4) of r and of mu [C][d] (no transposed copy), six column tiles for
//          C = 90 padded to 96; the A pieces of a row tile are loaded once and kept for all column tiles
// Rows are unit vectors already (the normalisation is the same work in both forms).  Prints the median time of each form over
// `reps` launches and the largest difference of the two results.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ubench/vmf_logits.hip -o tools/ubench/bin/vmf_logits ; run on the GPU:
//   vmf_logits [rows = 73469] [d = 64] [C = 90]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int MAX_D = 256;

// out [m][Cp]; muT [d][Cp]
__global__ __launch_bounds__(256) void logits_valu(const float* R, const float* muT, const float* kappa, const float* logz, float* out,
                                                   int m, int d, int C, int Cp) {
    __shared__ float rs[4][MAX_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int rr = 0; rr < 4; ++rr) {
        const int i = blockIdx.x * 16 + wave * 4 + rr;          // the same for the whole wave
        if (i >= m) continue;
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < d; k += 64) rs[wave][k] = R[(long long)i * d + k];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = lane + 64 * q;
            if (c >= C) continue;
            float acc = 0.f;
#pragma unroll 8
            for (int j = 0; j < d; ++j) acc += muT[(long long)j * Cp + c] * rs[wave][j];
            out[(long long)i * Cp + c] = logz[c] + kappa[c] * acc;
        }
    }
}

// out [m][Cp]; mu [Cp][d] (zero rows beyond C); d a multiple of 16, Cp of 16
template <int NKC>
__global__ __launch_bounds__(256) void logits_mfma(const float* R, const float* mu, const float* kappa, const float* logz, float* out,
                                                   int m, int C, int Cp) {
    constexpr int d = 16 * NKC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x * 4 + wave) * 16;
    if (row0 >= m) return;
    const int row = row0 + (lane & 15), kp = 4 * (lane >> 4);
    f32x4 a[NKC];
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
        a[kc] = row < m ? *reinterpret_cast<const f32x4*>(R + (long long)row * d + kc * 16 + kp) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < Cp / 16; ++t) {
        const int col = t * 16 + (lane & 15);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(mu + (long long)col * d + kc * 16 + kp);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kc][s], b[s], acc, 0, 0, 0);
        }
        const float kap = kappa[col], lz = logz[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int orow = row0 + 4 * (lane >> 4) + r;
            if (orow < m && col < C) out[(long long)orow * Cp + col] = lz + kap * acc[r];
        }
    }
}

int main(int argc, char** argv) {
    const int m = argc > 1 ? atoi(argv[1]) : 73469, d = argc > 2 ? atoi(argv[2]) : 64, C = argc > 3 ? atoi(argv[3]) : 90, reps = 21;
    if (m < 1 || d % 16 || d < 16 || d > 64 || C < 1 || C > 128) { printf("rows >= 1, d in {16, 32, 48, 64}, C <= 128\n"); return 2; }
    const int Cp = (C + 15) / 16 * 16;
    std::vector<float> R((size_t)m * d), mu((size_t)Cp * d, 0.f), muT((size_t)d * Cp, 0.f), kappa(Cp, 0.f), logz(Cp, 0.f);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.f / 8388608.f) - 1.f; };
    auto unit = [&](float* v) { double n = 0; for (int k = 0; k < d; ++k) n += (double)v[k] * v[k]; n = std::sqrt(n); for (int k = 0; k < d; ++k) v[k] = (float)(v[k] / n); };
    for (auto& v : R) v = rnd();
    for (int i = 0; i < m; ++i) unit(&R[(size_t)i * d]);
    for (int c = 0; c < C; ++c) {
        for (int k = 0; k < d; ++k) mu[(size_t)c * d + k] = rnd();
        unit(&mu[(size_t)c * d]);
        for (int k = 0; k < d; ++k) muT[(size_t)k * Cp + c] = mu[(size_t)c * d + k];
        kappa[c] = 10.f + 5.f * rnd(); logz[c] = 40.f + rnd();
    }
    float *dR, *dmu, *dmuT, *dk, *dz, *o1, *o2;
    CHECK(hipMalloc(&dR, R.size() * 4)); CHECK(hipMalloc(&dmu, mu.size() * 4)); CHECK(hipMalloc(&dmuT, muT.size() * 4));
    CHECK(hipMalloc(&dk, Cp * 4)); CHECK(hipMalloc(&dz, Cp * 4));
    CHECK(hipMalloc(&o1, (size_t)m * Cp * 4)); CHECK(hipMalloc(&o2, (size_t)m * Cp * 4));
    CHECK(hipMemcpy(dR, R.data(), R.size() * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(dmu, mu.data(), mu.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dmuT, muT.data(), muT.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dk, kappa.data(), Cp * 4, hipMemcpyHostToDevice)); CHECK(hipMemcpy(dz, logz.data(), Cp * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(o1, 0, (size_t)m * Cp * 4)); CHECK(hipMemset(o2, 0, (size_t)m * Cp * 4));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    auto valu = [&]() { hipLaunchKernelGGL(logits_valu, dim3((m + 15) / 16), dim3(256), 0, 0, dR, dmuT, dk, dz, o1, m, d, C, Cp); };
    auto mfma = [&]() {
        const dim3 g((m + 63) / 64), b(256);
        switch (d / 16) {
            case 1: hipLaunchKernelGGL(logits_mfma<1>, g, b, 0, 0, dR, dmu, dk, dz, o2, m, C, Cp); break;
            case 2: hipLaunchKernelGGL(logits_mfma<2>, g, b, 0, 0, dR, dmu, dk, dz, o2, m, C, Cp); break;
            case 3: hipLaunchKernelGGL(logits_mfma<3>, g, b, 0, 0, dR, dmu, dk, dz, o2, m, C, Cp); break;
            default: hipLaunchKernelGGL(logits_mfma<4>, g, b, 0, 0, dR, dmu, dk, dz, o2, m, C, Cp); break;
        }
    };
    std::vector<float> tv, tm;
    for (int it = 0; it < reps + 3; ++it) {                     // alternated; the first three rounds warm up
        float ms;
        CHECK(hipEventRecord(e0)); valu(); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 3) tv.push_back(ms * 1e3f);
        CHECK(hipEventRecord(e0)); mfma(); CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 3) tm.push_back(ms * 1e3f);
    }
    CHECK(hipGetLastError());
    std::vector<float> h1((size_t)m * Cp), h2((size_t)m * Cp);
    CHECK(hipMemcpy(h1.data(), o1, h1.size() * 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h2.data(), o2, h2.size() * 4, hipMemcpyDeviceToHost));
    double diff = 0, big = 0;
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < C; ++c) {
            diff = std::max(diff, (double)std::fabs(h1[(size_t)i * Cp + c] - h2[(size_t)i * Cp + c]));
            big = std::max(big, (double)std::fabs(h1[(size_t)i * Cp + c]));
        }
    std::sort(tv.begin(), tv.end()); std::sort(tm.begin(), tm.end());
    printf("vmf logits, %d rows x d %d x C %d (%.2f GFLOP, %.1f MB written): largest |valu - mfma| %.2e at a largest |l| of %.1f\n", m, d, C,
           2.0 * m * d * C * 1e-9, (double)m * Cp * 4e-6, diff, big);
    printf("  valu  %8.1f us (%8.1f .. %8.1f)\n  mfma  %8.1f us (%8.1f .. %8.1f)\n", tv[reps / 2], tv.front(), tv.back(), tm[reps / 2], tm.front(), tm.back());
    return 0;
}
