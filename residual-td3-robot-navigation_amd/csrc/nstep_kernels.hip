// nstep_kernels.hip — multi-step returns (DDPGfD, Rainbow, D4PG): the cut marks beside the
// replay ring (nav_nstep_stamp) and the gather that builds one epoch's critic batch as n-step
// rows (nav_nstep_rows). The successor of ring row k for the same env sits at the fixed stride
// n_envs, so a staged row {s, a, R_m, s_{t+m}, 1 - g^(m-1)} is one gather; the unchanged critic
// row kernels then form y = R_m + (gamma * min Q') * (1.0f - staged[7]): their effective discount
// gamma * fl32(1.0f - staged[7]) is exact for m == 1 (staged[7] is 0 or 1) and within one f32
// rounding of gamma^m for m > 1.
// A translation unit of its own: every other object of libnavenv.so compiles from the source it
// had before.
#include <utility>

#include "nav_device.h"

namespace {

using namespace nav;

struct NstepArgs {
    const float4* rows;   // the ring, two float4 per row
    const uint8_t* cut;   // [capacity]
    int64_t capacity, size, position;
    int64_t stride_mod;   // stride % capacity: k_j = k_{j-1} + stride_mod, one wrap at most
    int64_t stride_head;  // min(stride, capacity): j * stride_head > age exactly when j * stride is
    double g;             // (double)gamma
    int64_t B;
    const int64_t* idx;
    uint32_t s0, s1, ctr;
    float4* staged;
    int32_t* steps;
};

__global__ __launch_bounds__(kBlock) void k_nstep_stamp(uint8_t* __restrict__ cut,
                                                        int64_t capacity, int64_t pos, int64_t n,
                                                        const uint8_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int64_t k = pos + i;  // pos < capacity and i < n <= capacity: one wrap at most
    if (k >= capacity) k -= capacity;
    cut[k] = (uint8_t)((flags[i] >> 3) & 1u);
}

// One thread per batch row. Every successor address follows from k0, so all N high halves and
// cut bytes are loaded before the horizon is resolved (independent loads, not a chain); m, R and
// the last row are then picked in registers by fully unrolled selects.
template <int N>
__global__ __launch_bounds__(kBlock) void k_nstep_rows(NstepArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.B) return;
    int64_t k0;
    if (a.idx) {
        k0 = a.idx[b];
    } else {
        const uint4 w = philox((uint32_t)b, 0u, NAV_TAG_SAMPLE, 2u * a.ctr, a.s0, a.s1);
        k0 = (int64_t)(((uint64_t)w.x * (uint64_t)a.size) >> 32);
    }
    int64_t age = a.position - 1 - k0;  // rows written after k0
    if (age < 0) age += a.capacity;
    const float4 lo = a.rows[2 * k0];
    float4 hi[N];
    uint8_t c[N];
    int64_t k = k0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        hi[j] = a.rows[2 * k + 1];
        c[j] = a.cut[k];
        k += a.stride_mod;
        if (k >= a.capacity) k -= a.capacity;
    }
    int m = N;  // the smallest j >= 1 that ends the horizon
#pragma unroll
    for (int j = N - 1; j >= 1; --j)
        if (c[j - 1] != 0 || (int64_t)j * a.stride_head > age) m = j;
    double R = (double)hi[0].x, gp = 1.0, gl = 1.0;
    float4 last = hi[0];
#pragma unroll
    for (int j = 1; j < N; ++j) {  // selects, not branches: no load waits behind a condition
        gp *= a.g;
        const bool in = j < m;
        const double t = R + gp * (double)hi[j].x;
        R = in ? t : R;
        last.y = in ? hi[j].y : last.y;
        last.z = in ? hi[j].z : last.z;
        last.w = in ? hi[j].w : last.w;
        gl = in ? gp : gl;
    }
    a.staged[2 * b] = lo;
    a.staged[2 * b + 1] =
        make_float4((float)R, last.y, last.z, last.w != 0.f ? 1.0f : (float)(1.0 - gl));
    if (a.steps) a.steps[b] = m;
}

typedef void (*NstepKernel)(NstepArgs);
template <int... Ns>
NstepKernel nstep_kernel(int n, std::integer_sequence<int, Ns...>) {
    static const NstepKernel table[] = {k_nstep_rows<Ns + 1>...};
    return table[n - 1];
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int nav_nstep_stamp(uint8_t* cut, int64_t capacity, int64_t pos, int64_t n,
                               const uint8_t* flags, void* stream) {
    if (!cut || !flags || capacity < 1 || n < 0 || n > capacity || pos < 0 || pos >= capacity)
        return NAV_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_nstep_stamp, dim3(blocks_for(n)), dim3(kBlock), 0, S(stream), cut,
                       capacity, pos, n, flags);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nav_nstep_rows(const nav_replay* replay, const uint8_t* cut, int64_t size,
                              int64_t position, int64_t stride, int32_t n_step, float gamma,
                              int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                              uint32_t counter, float* staged, int32_t* steps, void* stream) {
    if (!replay || !replay->rows || !cut || !staged || size < 1 || size > replay->capacity ||
        size > ((int64_t)1 << 32) || position < 0 || position >= replay->capacity ||
        (size < replay->capacity && position != size) || stride < 1 || n_step < 1 ||
        n_step > NAV_NSTEP_MAX || B < 1 || !(gamma >= 0.f && gamma <= 1.f))
        return NAV_EINVAL;
    const int64_t cap = replay->capacity;
    NstepArgs a;
    a.rows = reinterpret_cast<const float4*>(replay->rows);
    a.cut = cut;
    a.capacity = cap;
    a.size = size;
    a.position = position;
    a.stride_mod = stride % cap;
    a.stride_head = stride < cap ? stride : cap;
    a.g = (double)gamma;
    a.B = B;
    a.idx = idx;
    a.s0 = seed_lo;
    a.s1 = seed_hi;
    a.ctr = counter;
    a.staged = reinterpret_cast<float4*>(staged);
    a.steps = steps;
    hipLaunchKernelGGL(nstep_kernel(n_step, std::make_integer_sequence<int, NAV_NSTEP_MAX>()),
                       dim3(blocks_for(B)), dim3(kBlock), 0, S(stream), a);
    NAV_CHECK_LAUNCH();
    return 0;
}
