// demo_reward.hip — the demo-proximity term of the reward (robot.py:749-760) as passes of their
// own over the envs a tick flagged: brute force over a group's demonstration points
// (nav_demo_reward), through the exact bucketed index of demo_index.hip
// (nav_demo_reward_indexed), and the bare minimum distance of arbitrary points (nav_demo_min).
#include "env_host.h"

namespace {

// robot.py:753 demo-proximity min distance, f64 exactly as scipy's cdist (dx*dx + dy*dy, no
// fma; sqrt is monotone and correctly rounded, so sqrt(min) == min(sqrt)). One wave = 64 envs of
// one group; every lane tests the same point at the same time, so the points are read with
// wave-uniform (scalar-unit) loads straight into SGPRs — no LDS staging, no bank traffic — and
// four independent min chains keep the f64 pipe busy. A workgroup = kDemoSplit waves over the
// SAME 64 envs, each scanning 1/kDemoSplit of the points (4 waves per SIMD hide the scalar-cache
// latency), combined through LDS.
constexpr int kDemoEnvs = 64;
constexpr int kDemoSplit = 8;
constexpr int kDemoBlock = kDemoEnvs * kDemoSplit;

NAV_DEV double demo_min_uniform(const double* __restrict__ d, int m, double x, double y) {
    double b0 = __builtin_inf(), b1 = b0, b2 = b0, b3 = b0;
    int j = 0;
    for (; j + 4 <= m; j += 4) {
        const double* q = d + 2 * j;
        const double v0 = sqd(x, y, q[0], q[1]), v1 = sqd(x, y, q[2], q[3]);
        const double v2 = sqd(x, y, q[4], q[5]), v3 = sqd(x, y, q[6], q[7]);
        // fmin == (v < b ? v : b) here: no NaN among the distances
        b0 = fmin(v0, b0);
        b1 = fmin(v1, b1);
        b2 = fmin(v2, b2);
        b3 = fmin(v3, b3);
    }
    for (; j < m; ++j) b0 = fmin(sqd(x, y, d[2 * j], d[2 * j + 1]), b0);
    return fmin(fmin(b0, b1), fmin(b2, b3));
}

__global__ __launch_bounds__(kDemoBlock) void k_demo_reward(nav_params p, int64_t n,
                                                            const double2* __restrict__ ns,
                                                            const double* __restrict__ gterm,
                                                            const uint8_t* __restrict__ flags,
                                                            const double* __restrict__ demo,
                                                            const int64_t* __restrict__ off,
                                                            int64_t m_shared, int32_t epg,
                                                            float* __restrict__ rows,
                                                            int64_t cap, int64_t base,
                                                            double* __restrict__ reward_out) {
    __shared__ double part[kDemoSplit][kDemoEnvs];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * kDemoEnvs;
    const int64_t e = e0 + lane;
    const bool live = e < n;
    const uint8_t f = live ? flags[e] : 0;
    const bool want = live && (f & F_DEMO);
    if (!__syncthreads_or(want ? 1 : 0)) return;
    double x = 0.0, y = 0.0;
    if (live) {
        const double2 s = ns[e];
        x = s.x;
        y = s.y;
    }
    const int64_t last = e0 + kDemoEnvs - 1 < n ? e0 + kDemoEnvs - 1 : n - 1;
    const int64_t g0 = off ? e0 / epg : 0, g1 = off ? last / epg : 0;
    double best;
    if (g0 == g1) {  // the 64 envs share one group: wave-uniform scalar loads
        const int64_t lo = off ? off[g0] : 0, hi = off ? off[g0 + 1] : m_shared;
        const int64_t m = hi - lo, per = (m + kDemoSplit - 1) / kDemoSplit;
        const int64_t a = lo + wv * per, b = a + per < hi ? a + per : hi;
        best = a < b ? demo_min_uniform(demo + 2 * a, (int)(b - a), x, y) : __builtin_inf();
    } else if (wv == 0) {
        const int64_t g = live ? e / epg : g0;
        best = demo_min_global(reinterpret_cast<const double2*>(demo) + off[g],
                               off[g + 1] - off[g], x, y);
    } else {
        best = __builtin_inf();
    }
    part[wv][lane] = best;
    __syncthreads();
    if (wv != 0 || !want) return;
#pragma unroll
    for (int k = 1; k < kDemoSplit; ++k) best = fmin(best, part[k][lane]);
    // robot.py:756-760 then the stuck penalty of robot.py:667-669
    const double mn = sqrt(best);
    double r = gterm[e] + p.demo_factor * (-mn);
    if (f & F_STUCK) r -= p.stuck_penalty;
    const int64_t slot = (base + e) % cap;
    rows[slot * NAV_ROW + 4] = (float)r;
    if (reward_out) reward_out[e] = r;
}

// The same for a handful of envs (the N = 1 drop-in's process_transition): one workgroup per env,
// its threads over the demonstration points (a lane per point instead of a lane per env), the
// minimum by wave shuffles and LDS — the same f64 minimum over the same set, so the same reward.
__global__ __launch_bounds__(kDemoBlock) void k_demo_reward_few(nav_params p,
                                                                const double2* __restrict__ ns,
                                                                const double* __restrict__ gterm,
                                                                const uint8_t* __restrict__ flags,
                                                                const double* __restrict__ demo,
                                                                const int64_t* __restrict__ off,
                                                                int64_t m_shared, int32_t epg,
                                                                float* __restrict__ rows,
                                                                int64_t cap, int64_t base,
                                                                double* __restrict__ reward_out) {
    __shared__ double part[kDemoBlock / 64];
    const int64_t e = blockIdx.x;
    const uint8_t f = flags[e];
    if (!(f & F_DEMO)) return;  // workgroup-uniform
    const double2 s = ns[e];
    const int64_t g = off ? e / epg : 0;
    const int64_t lo = off ? off[g] : 0, hi = off ? off[g + 1] : m_shared;
    double best = __builtin_inf();
    for (int64_t j = lo + threadIdx.x; j < hi; j += kDemoBlock)
        best = fmin(sqd(s.x, s.y, demo[2 * j], demo[2 * j + 1]), best);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmin(best, __shfl_xor(best, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < kDemoBlock / 64; ++k) best = fmin(best, part[k]);
    // robot.py:756-760 then the stuck penalty of robot.py:667-669 (k_demo_reward's order)
    const double mn = sqrt(best);
    double r = gterm[e] + p.demo_factor * (-mn);
    if (f & F_STUCK) r -= p.stuck_penalty;
    const int64_t slot = (base + e) % cap;
    rows[slot * NAV_ROW + 4] = (float)r;
    if (reward_out) reward_out[e] = r;
}

// The demo-proximity term through the index: lane = env, its cell = the index cell of s'.
__global__ __launch_bounds__(kBlock) void k_demo_reward_idx(nav_params p, int64_t n,
                                                            const double2* __restrict__ ns,
                                                            const double* __restrict__ gterm,
                                                            const uint8_t* __restrict__ flags,
                                                            DemoIdx d, float* __restrict__ rows,
                                                            int64_t cap, int64_t base,
                                                            double* __restrict__ reward_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const uint8_t f = flags[e];
    if (!(f & F_DEMO)) return;
    const double r = demo_reward_of(p, gterm[e], demo_min2_idx(d, e, ns[e]), (f & F_STUCK) != 0);
    const int64_t slot = (base + e) % cap;
    rows[slot * NAV_ROW + 4] = (float)r;
    if (reward_out) reward_out[e] = r;
}

// robot.py:753 min_j ||p_i - d_j|| for arbitrary points (scipy cdist semantics).
__global__ __launch_bounds__(kBlock) void k_demo_min(const double2* __restrict__ pts, int64_t n,
                                                     const double2* __restrict__ demo, int64_t m,
                                                     double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double2 s = pts[i];
    out[i] = sqrt(demo_min_global(demo, m, s.x, s.y));
}

// block_stats' reward column after a separate demo pass (nav_demo_reward(_indexed) with
// block_stats): the row of every 64 envs that hold a flagged env is summed again from the pushed
// rewards (the replay rows, now final) — the same wave tree over the same floats as the tick
// that runs the demo pass in its own launch, so every launch form reports the pushed reward.
__global__ __launch_bounds__(kBlock) void k_restat_reward(int64_t n, const uint8_t* __restrict__ flags,
                                                          const float* __restrict__ rows,
                                                          int64_t cap, int64_t base,
                                                          float* __restrict__ block_stats) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = e < n;
    const bool flagged = live && (flags[e] & F_DEMO);
    if (!__any(flagged)) return;  // wave-uniform
    const float r = live ? rows[((base + e) % cap) * NAV_ROW + 4] : 0.f;
    const float v = wave_sum(r);
    if ((threadIdx.x & 63) == 0) block_stats[(e >> 6) * 8] = v;
}

// the tail of both demo passes: block_stats (nullable) of the rewards they pushed
int restat(int64_t n, const uint8_t* flags, const nav_replay* replay, int64_t base,
           float* block_stats, void* stream) {
    if (!block_stats) return 0;
    return launch_items(k_restat_reward, n, stream, n, flags, replay->rows, replay->capacity, base,
                        block_stats);
}

}  // namespace

extern "C" {

int nav_demo_reward(const nav_params* p, int64_t n, const double* next_state,
                    const double* goal_term, const uint8_t* flags, const double* demo_xy,
                    const int64_t* demo_off, int64_t m, int32_t epg, const nav_replay* replay,
                    int64_t replay_base, double* reward_out, float* block_stats, void* stream) {
    if (!p || n < 0 || !ring_ok(replay, replay_base)) return NAV_EINVAL;
    if (n && (!next_state || !goal_term || !flags)) return NAV_EINVAL;
    if (demo_off && epg <= 0) return NAV_EINVAL;
    if (!demo_off && m > 0 && !demo_xy) return NAV_EINVAL;
    if (n == 0 || (!demo_off && m == 0)) return 0;
    const int64_t base = ring_origin(replay, replay_base);
    const int st =
        n <= 8  // a lane per point (the N = 1 drop-in): 81 us -> a few per call
            ? launch(k_demo_reward_few, dim3((unsigned)n), dim3(kDemoBlock), stream, *p,
                     d2(next_state), goal_term, flags, demo_xy, demo_off, m, epg > 0 ? epg : 1,
                     replay->rows, replay->capacity, base, reward_out)
            : launch(k_demo_reward, dim3((unsigned)((n + kDemoEnvs - 1) / kDemoEnvs)),
                     dim3(kDemoBlock), stream, *p, n, d2(next_state), goal_term, flags, demo_xy,
                     demo_off, m, epg > 0 ? epg : 1, replay->rows, replay->capacity, base,
                     reward_out);
    return st ? st : restat(n, flags, replay, base, block_stats, stream);
}

int nav_demo_reward_indexed(const nav_params* p, int64_t n, const double* next_state,
                            const double* goal_term, const uint8_t* flags, const double* demo_xy,
                            const int64_t* demo_off, int32_t envs_per_group,
                            const int64_t* cell_start, const int32_t* cand,
                            const nav_replay* replay, int64_t replay_base, double* reward_out,
                            float* block_stats, void* stream) {
    if (!p || n < 0 || !ring_ok(replay, replay_base) || (demo_off && envs_per_group <= 0))
        return NAV_EINVAL;
    if (n == 0) return 0;
    if (!next_state || !goal_term || !flags || !demo_xy || !cell_start || !cand)
        return NAV_EINVAL;
    const int64_t base = ring_origin(replay, replay_base);
    const DemoIdx d = demo_idx(demo_xy, demo_off, envs_per_group, cell_start, cand);
    const int st = launch_items(k_demo_reward_idx, n, stream, *p, n, d2(next_state), goal_term,
                                flags, d, replay->rows, replay->capacity, base, reward_out);
    return st ? st : restat(n, flags, replay, base, block_stats, stream);
}

int nav_demo_min(const double* points, int64_t n, const double* demo_xy, int64_t m,
                 double* out, void* stream) {
    if (n < 0 || m < 1 || (n && (!points || !demo_xy || !out))) return NAV_EINVAL;
    if (n == 0) return 0;
    return launch_items(k_demo_min, n, stream, d2(points), n, d2(demo_xy), m, out);
}

}  // extern "C"
