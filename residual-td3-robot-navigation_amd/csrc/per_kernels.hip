// per_kernels.hip — prioritised replay (Schaul et al. 2016, the proportional variant): the
// priority store beside the replay ring, its sum hierarchy, the device-side sampler with the
// importance weights, and the priority update from the critics' |TD errors| (nav_per_*).
// Priorities are u32 fixed point (16 fractional bits) and every sum an exact u64, so a draw is a
// pure function of the stored integers and the Philox words, whatever the hierarchy's shape.
// A translation unit of its own: every other object of libnavenv.so compiles from the source it
// had before.
#include "nav_device.h"

namespace {

using namespace nav;

constexpr int kGroup = 32;                 // rows per level-0 sum
constexpr int kChunk = 1024;               // rows per level-1 sum (one workgroup of k_per_sums)
constexpr int kGroupsPerChunk = kChunk / kGroup;
constexpr uint32_t kOne = 65536u;          // priority 1.0
constexpr uint32_t kMaxPri = 0x7FFFFFFFu;  // 2^31 - 1

// the workspace (u64 words) for n1k = ceil(capacity / 1024) chunks:
//   [0] the total S, [1] reserved
//   p1k  [n1k + 1]  exclusive prefix of the chunk sums; entry `used chunks` = S
//   s1k  [n1k]      chunk sums
//   m1k  [n1k]      chunk minima (over rows < size)
//   s32  [n1k * 32] 32-row sums (groups past `size` hold 0)
struct Layout {
    int64_t n1k;
    __host__ __device__ explicit Layout(int64_t capacity) : n1k((capacity + kChunk - 1) / kChunk) {}
    __host__ __device__ int64_t p1k() const { return 2; }
    __host__ __device__ int64_t s1k() const { return p1k() + n1k + 1; }
    __host__ __device__ int64_t m1k() const { return s1k() + n1k; }
    __host__ __device__ int64_t s32() const { return m1k() + n1k; }
    __host__ __device__ int64_t count() const { return s32() + n1k * kGroupsPerChunk; }
};

NAV_DEV uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void k_per_init(nav_per per) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k < per.capacity) per.pri[k] = 0u;
    if (k < 4) per.stat[k] = k == 0 ? kOne : 0u;
}

__global__ __launch_bounds__(kBlock) void k_per_stamp(nav_per per, int64_t pos, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int64_t k = pos + i;  // pos < capacity and i < n <= capacity: one wrap at most
    if (k >= per.capacity) k -= per.capacity;
    per.pri[k] = per.stat[0];
}

// one workgroup per chunk of 1024 rows: pass k of thread t reads row chunk * 1024 + k * 256 + t
// (coalesced), so a 32-row group is one half-wave of one pass
__global__ __launch_bounds__(kBlock) void k_per_sums(nav_per per, int64_t size) {
    __shared__ uint64_t wsum[kBlock / 64];
    __shared__ uint32_t wmin[kBlock / 64];
    const Layout lay(per.capacity);
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x, row0 = chunk * kChunk;
    uint64_t tot = 0;
    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < kChunk / kBlock; ++k) {
        const int64_t r = row0 + k * kBlock + tid;
        uint64_t v = 0;
        if (r < size) {
            const uint32_t p = per.pri[r];
            v = p;
            mn = min(mn, p);
        }
        tot += v;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
        if ((tid & 31) == 0)
            per.sums[lay.s32() + chunk * kGroupsPerChunk + k * (kBlock / kGroup) + tid / kGroup] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tot += shfl_xor_u64(tot, o);
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    }
    if ((tid & 63) == 0) {
        wsum[tid >> 6] = tot;
        wmin[tid >> 6] = mn;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t s = 0;
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) {
            s += wsum[k];
            m = min(m, wmin[k]);
        }
        per.sums[lay.s1k() + chunk] = s;
        per.sums[lay.m1k() + chunk] = m;
    }
}

// one workgroup: the exclusive prefix of the `used` chunk sums (256 per pass, a running carry),
// the total and the minimum
__global__ __launch_bounds__(kBlock) void k_per_scan(nav_per per, int64_t used) {
    __shared__ uint64_t buf[kBlock];
    __shared__ uint32_t mbuf[kBlock];
    const Layout lay(per.capacity);
    const int tid = threadIdx.x;
    uint64_t carry = 0;
    uint32_t mn = 0xFFFFFFFFu;
    for (int64_t c0 = 0; c0 < used; c0 += kBlock) {
        const int64_t c = c0 + tid;
        const uint64_t v = c < used ? per.sums[lay.s1k() + c] : 0;
        if (c < used) mn = min(mn, (uint32_t)per.sums[lay.m1k() + c]);
        buf[tid] = v;
        __syncthreads();
        for (int o = 1; o < kBlock; o <<= 1) {  // Hillis-Steele inclusive scan
            const uint64_t add = tid >= o ? buf[tid - o] : 0;
            __syncthreads();
            buf[tid] += add;
            __syncthreads();
        }
        if (c < used) per.sums[lay.p1k() + c] = carry + buf[tid] - v;
        carry += buf[kBlock - 1];
        __syncthreads();
    }
    mbuf[tid] = mn;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (tid < o) mbuf[tid] = min(mbuf[tid], mbuf[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        per.sums[lay.p1k() + used] = carry;
        per.sums[0] = carry;
        per.stat[1] = mbuf[0];
    }
}

// the row of target t: min{k : P_k > t}. Chunk by binary search over the exclusive prefixes,
// then the chunk's 32-row sums, then the group's rows; every comparison is on exact integers.
NAV_DEV int64_t per_find(const nav_per& per, const Layout& lay, int64_t size, uint64_t t) {
    const uint64_t* p1k = per.sums + lay.p1k();
    int64_t lo = 0, hi = (size + kChunk - 1) / kChunk;  // the largest c in [lo, hi) with p1k[c] <= t
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p1k[mid] <= t) lo = mid;
        else hi = mid;
    }
    uint64_t rem = t - p1k[lo];
    // the group, then the row: all 32 values loaded at once (independent loads, not a chain of
    // 31 dependent ones), then the count of leading running sums that rem still reaches. The
    // running sums do not decrease, so that count is where a one-by-one subtraction stops.
    const uint64_t* s32 = per.sums + lay.s32() + lo * kGroupsPerChunk;
    uint64_t s[kGroupsPerChunk];
#pragma unroll
    for (int i = 0; i < kGroupsPerChunk; ++i) s[i] = s32[i];
    int g = 0;
    uint64_t acc = 0, off = 0;
#pragma unroll
    for (int i = 0; i < kGroupsPerChunk - 1; ++i) {
        acc += s[i];
        if (rem >= acc) {
            g = i + 1;
            off = acc;
        }
    }
    rem -= off;
    const int64_t base = (lo * kGroupsPerChunk + g) * kGroup;
    uint32_t p[kGroup];  // rows at or beyond size: not read, no mass
#pragma unroll
    for (int i = 0; i < kGroup; ++i) p[i] = base + i < size ? per.pri[base + i] : 0u;
    int j = 0;
    acc = 0;
#pragma unroll
    for (int i = 0; i < kGroup - 1; ++i) {
        acc += p[i];
        if (rem >= acc) j = i + 1;
    }
    return min(base + j, size - 1);
}

// grid.y = 0: the critic's draw and weight, 1: the actor's draw
__global__ __launch_bounds__(kBlock) void k_per_sample(nav_per per, int64_t size, int64_t B,
                                                       uint32_t seed_lo, uint32_t seed_hi,
                                                       uint32_t counter, float beta,
                                                       int64_t* __restrict__ idx_critic,
                                                       float* __restrict__ w_critic,
                                                       int64_t* __restrict__ idx_actor) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int which = blockIdx.y;
    int64_t* out = which ? idx_actor : idx_critic;
    if (b >= B || !out) return;
    const Layout lay(per.capacity);
    const uint4 w = philox((uint32_t)b, 0u, NAV_TAG_PER, 2u * counter + (uint32_t)which, seed_lo,
                           seed_hi);
    const uint64_t r64 = ((uint64_t)w.y << 32) | w.x;
    const uint64_t t = __umul64hi(r64, per.sums[0]);
    const int64_t k = per_find(per, lay, size, t);
    out[b] = k;
    if (which == 0 && w_critic)
        w_critic[b] = (float)pow((double)per.stat[1] / (double)per.pri[k], (double)beta);
}

NAV_DEV uint32_t per_priority(float td1, float td2, float alpha, float eps) {
    const double m = 0.5 * (fabs((double)td1) + fabs((double)td2)) + (double)eps;
    const double v = floor(pow(m, (double)alpha) * 65536.0 + 0.5);
    if (!(v >= 1.0)) return 1u;  // NaN too
    return v >= 2147483647.0 ? kMaxPri : (uint32_t)v;
}

// two launches: the sampled rows' old values go, then the maximum over each row's new values
__global__ __launch_bounds__(kBlock) void k_per_update_clear(nav_per per, int64_t B,
                                                             const int64_t* __restrict__ idx) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const int64_t k = idx[b];
    if (k >= 0 && k < per.capacity) per.pri[k] = 0u;
}

__global__ __launch_bounds__(kBlock) void k_per_update_max(nav_per per, int64_t B,
                                                           const int64_t* __restrict__ idx,
                                                           const float* __restrict__ td1,
                                                           const float* __restrict__ td2,
                                                           float alpha, float eps) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t q = 0u;
    if (b < B) {
        q = per_priority(td1[b], td2[b], alpha, eps);
        const int64_t k = idx[b];
        if (k >= 0 && k < per.capacity) atomicMax(&per.pri[k], q);
    }
    uint32_t mx = q;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&per.stat[0], mx);
}

bool per_ok(const nav_per* per) {
    return per && per->pri && per->sums && per->stat && per->capacity >= 1;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int64_t nav_per_sums_count(int64_t capacity) {
    if (capacity < 1) return NAV_EINVAL;
    return Layout(capacity).count();
}

extern "C" int nav_per_init(const nav_per* per, void* stream) {
    if (!per_ok(per)) return NAV_EINVAL;
    hipLaunchKernelGGL(k_per_init, dim3(blocks_for(per->capacity)), dim3(kBlock), 0, S(stream),
                       *per);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nav_per_stamp(const nav_per* per, int64_t pos, int64_t n, void* stream) {
    if (!per_ok(per) || n < 0 || n > per->capacity || pos < 0 || pos >= per->capacity)
        return NAV_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_per_stamp, dim3(blocks_for(n)), dim3(kBlock), 0, S(stream), *per, pos, n);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nav_per_sums(const nav_per* per, int64_t size, void* stream) {
    if (!per_ok(per) || size < 1 || size > per->capacity) return NAV_EINVAL;
    const int64_t used = (size + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(k_per_sums, dim3((unsigned)used), dim3(kBlock), 0, S(stream), *per, size);
    hipLaunchKernelGGL(k_per_scan, dim3(1), dim3(kBlock), 0, S(stream), *per, used);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nav_per_sample(const nav_per* per, int64_t size, int64_t B, uint32_t seed_lo,
                              uint32_t seed_hi, uint32_t counter, float beta,
                              int64_t* idx_critic, float* w_critic, int64_t* idx_actor,
                              void* stream) {
    if (!per_ok(per) || size < 1 || size > per->capacity || B < 1 || !(beta >= 0.f) ||
        (w_critic && !idx_critic))
        return NAV_EINVAL;
    if (!idx_critic && !idx_actor) return 0;
    hipLaunchKernelGGL(k_per_sample, dim3(blocks_for(B), 2u), dim3(kBlock), 0, S(stream), *per,
                       size, B, seed_lo, seed_hi, counter, beta, idx_critic, w_critic, idx_actor);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" int nav_per_update(const nav_per* per, int64_t B, const int64_t* idx, const float* td1,
                              const float* td2, float alpha, float eps, void* stream) {
    if (!per_ok(per) || B < 1 || !idx || !td1 || !td2 || !(alpha > 0.f) || !(eps >= 0.f))
        return NAV_EINVAL;
    hipLaunchKernelGGL(k_per_update_clear, dim3(blocks_for(B)), dim3(kBlock), 0, S(stream), *per,
                       B, idx);
    hipLaunchKernelGGL(k_per_update_max, dim3(blocks_for(B)), dim3(kBlock), 0, S(stream), *per, B,
                       idx, td1, td2, alpha, eps);
    NAV_CHECK_LAUNCH();
    return 0;
}
