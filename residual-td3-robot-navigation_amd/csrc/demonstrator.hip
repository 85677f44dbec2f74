// demonstrator.hip — what runs once at set-up time to make the demonstrations: open-loop
// rollouts through Environment.dynamics, the batched CEM planner (environment.py:140-179), the
// dynamics fields (nav.fields) and the augmented demonstration set (robot.py:771-824).
#include "env_host.h"

namespace {

// Batched open-loop rollouts through Environment.dynamics (the CEM demonstrator's inner loop,
// environment.py:151-165): lane = path, T sequential steps, state carried in f64; paths [P][T+1][2]
// f64; reward (nullable) = -||f32(s_T) - goal|| as compute_reward on the float32 planning_paths
// row (environment.py:164, 182-183).
__global__ __launch_bounds__(kBlock) void k_rollout(const float2* __restrict__ field, int64_t P,
                                                    int32_t T, const double2* __restrict__ start,
                                                    const double2* __restrict__ actions,
                                                    double2* __restrict__ paths,
                                                    const double* __restrict__ goal,
                                                    double* __restrict__ reward) {
    const int64_t pth = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pth >= P) return;
    double2 s = start[pth];
    paths[pth * (T + 1)] = s;
    for (int t = 0; t < T; ++t) {
        s = dynamics(field, s, actions[pth * T + t]);
        paths[pth * (T + 1) + t + 1] = s;
    }
    if (reward) {
        const double fx = (double)(float)s.x, fy = (double)(float)s.y;
        reward[pth] = -norm2(fx - goal[0], fy - goal[1]);
    }
}

// ---------------- batched CEM demonstrator (environment.py:140-179) ----------------
// n_prob independent CEM problems (one per group and demonstration), each P paths x T steps. One
// rollout launch per CEM iteration over every problem's paths (lane = path, state in f64 as the
// reference's planning_state), then one elite launch per iteration (workgroup = problem).
// Iteration 0 takes the +-5 actions drawn by np.random.choice, later ones
// a = mean[t] + std[t] * z in f64 (legacy normal = loc + scale * gauss) with z the standard
// normal draws; both are drawn on the host from each problem's numpy stream, in the reference's
// order, so the plans equal nav.Environment.get_demonstration's on the same stream.
__global__ __launch_bounds__(kBlock) void k_cem_rollout(const float2* __restrict__ field,
                                                        int32_t n_prob, int32_t P, int32_t T,
                                                        int32_t iter,
                                                        const double* __restrict__ region,
                                                        const double2* __restrict__ uni,
                                                        const double2* __restrict__ goal,
                                                        const double2* __restrict__ a0,
                                                        const double2* __restrict__ z,
                                                        const float2* __restrict__ mean,
                                                        const float2* __restrict__ stdv,
                                                        float2* __restrict__ actions,
                                                        float2* __restrict__ paths,
                                                        double* __restrict__ reward) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;  // problem * P + path
    if (i >= (int64_t)n_prob * P) return;
    const int64_t prob = i / P;
    // environment.py:150 get_random_robot_init_state (the same formula as nav_env_reset)
    const double* rg = region + 4 * prob;
    const double reg[4] = {rg[0], rg[1], rg[2], rg[3]};
    const double2 u = uni[prob];
    double2 s = region_sample(reg, u.x, u.y);
    const int64_t base = i * T;
    if (paths) paths[i * (T + 1)] = make_float2((float)s.x, (float)s.y);
    for (int t = 0; t < T; ++t) {
        double2 a;
        if (iter == 0) {
            a = a0[base + t];
        } else {
            const float2 m = mean[prob * T + t], sd = stdv[prob * T + t];
            const double2 zz = z[base + t];
            a = make_double2((double)m.x + (double)sd.x * zz.x, (double)m.y + (double)sd.y * zz.y);
        }
        actions[base + t] = make_float2((float)a.x, (float)a.y);  // planning_actions (float32)
        s = dynamics(field, s, a);
        if (paths) paths[i * (T + 1) + t + 1] = make_float2((float)s.x, (float)s.y);
    }
    // environment.py:164, 182-183 on the float32 planning_paths row
    const double2 g = goal[prob];
    reward[i] = -norm2((double)(float)s.x - g.x, (double)(float)s.y - g.y);
}

// ---------------- dynamics fields (environment.py:59-95 set_dynamics; nav.fields) ----------------
// nav.fields' construction on the device: per cell (i, j) of the x-major 100 x 100 grid the f64
// gradient noise of octave o at (i/100*o, j/100*o) from the unit gradient table g_o [o+1][o+1][2]
// (quintic fade, bilinear blend), speed cells = f32((n5 + .5 n10) + .25 n20), angle cells =
// f32(n5) (the same octave-5 values), each min-max normalised in f32 and the speed stretched by 1/(1 + exp(-10 (x - .5)))
// in f32 (the exp rounded from f64) — numpy's operation order, -ffp-contract=off. One 1024-thread workgroup (10 000 cells,
// block min / max in LDS); field out [100][100][2] (speed, angle) interleaved, the kernels'
// table layout.
constexpr int kFieldThreads = 1024;
NAV_DEV double grad_noise(const double* __restrict__ g, int oct, int i, int j) {
    const double x = ((double)i / 100.0) * oct, y = ((double)j / 100.0) * oct;
    const double xf = floor(x), yf = floor(y);
    const int x0 = (int)xf, y0 = (int)yf;
    const double fx = x - xf, fy = y - yf;
    const int w = oct + 1;
    auto dot = [&](int ix, int iy, double dx, double dy) {
        const double* v = g + ((int64_t)ix * w + iy) * 2;
        return v[0] * dx + v[1] * dy;
    };
    auto fade = [](double t) { return t * t * t * (t * (t * 6.0 - 15.0) + 10.0); };
    const double n00 = dot(x0, y0, fx, fy);
    const double n10 = dot(x0 + 1, y0, fx - 1.0, fy);
    const double n01 = dot(x0, y0 + 1, fx, fy - 1.0);
    const double n11 = dot(x0 + 1, y0 + 1, fx - 1.0, fy - 1.0);
    const double wx = fade(fx), wy = fade(fy);
    return (n00 * (1.0 - wx) + n10 * wx) * (1.0 - wy) + (n01 * (1.0 - wx) + n11 * wx) * wy;
}

NAV_DEV void block_minmax(float& mn, float& mx, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        red[2 * wv] = mn;
        red[2 * wv + 1] = mx;
    }
    __syncthreads();
    mn = red[0];
    mx = red[1];
    for (int w = 1; w < kFieldThreads / 64; ++w) {
        mn = fminf(mn, red[2 * w]);
        mx = fmaxf(mx, red[2 * w + 1]);
    }
}

__global__ __launch_bounds__(kFieldThreads) void k_fields(const double* __restrict__ g5,
                                                          const double* __restrict__ g10,
                                                          const double* __restrict__ g20,
                                                          float2* __restrict__ field) {
    constexpr int N = NAV_WORLD_CELLS * NAV_WORLD_CELLS;
    __shared__ float sp[N];
    __shared__ float an[N];
    __shared__ float red[2 * kFieldThreads / 64];
    float smn = __builtin_inff(), smx = -__builtin_inff(), amn = smn, amx = smx;
    for (int c = threadIdx.x; c < N; c += kFieldThreads) {
        const int i = c / NAV_WORLD_CELLS, j = c % NAV_WORLD_CELLS;
        // the angle's noise IS the speed's first term (environment.py:62 and :85: the same
        // PerlinNoise(octaves=5, seed) function), so one evaluation feeds both tables
        const double n5 = grad_noise(g5, 5, i, j);
        const double v = (n5 + 0.5 * grad_noise(g10, 10, i, j)) + 0.25 * grad_noise(g20, 20, i, j);
        const float fs = (float)v, fa = (float)n5;
        sp[c] = fs;
        an[c] = fa;
        smn = fminf(smn, fs);
        smx = fmaxf(smx, fs);
        amn = fminf(amn, fa);
        amx = fmaxf(amx, fa);
    }
    block_minmax(smn, smx, red);
    block_minmax(amn, amx, red);
    const float sr = smx - smn, ar = amx - amn;
    for (int c = threadIdx.x; c < N; c += kFieldThreads) {
        const float nrm = (sp[c] - smn) / sr;
        const float t = -10.0f * (nrm - 0.5f);
        // numpy's float32 exp is within an ulp of the correctly rounded value; the f64 exp
        // rounded to f32 is the correctly rounded value but for double-rounding cases
        const float speed = 1.0f / (1.0f + (float)exp((double)t));
        field[c] = make_float2(speed, (an[c] - amn) / ar);
    }
}

// Robot.process_demonstration's demonstration set (robot.py:694-698) with the augmentation of
// robot.py:771-824, one output point per thread: demo d's block is its T original states (f64 of
// the f32 CEM states), then per augmentation k the (T-1)*(steps+1) + 1 augmented states: for
// transition i and sub-step s < steps the float32 interpolation cur + f32(s+1)/(steps+1)*(nxt-cur)
// (numpy NEP 50: a python-float fraction times a float32 array stays float32, no fma) plus the
// state noise, at s = steps the current state plus noise, and finally the last state plus noise.
// noise [n_demo][n_aug][D], D = (T-1)(steps+1)*4 + 4: the augmentation's normal draws in the
// reference's order (per (i, s): state 2, action 2; then the last state 2, last action 2).
__global__ __launch_bounds__(kBlock) void k_demo_augment(int32_t n_demo, int32_t T, int32_t steps,
                                                         int32_t n_aug,
                                                         const float2* __restrict__ states,
                                                         const double* __restrict__ noise,
                                                         double2* __restrict__ out) {
    const int64_t per = steps + 1, A = (int64_t)(T - 1) * per + 1, Lp = T + n_aug * A;
    const int64_t D = (int64_t)(T - 1) * per * 4 + 4;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= (int64_t)n_demo * Lp) return;
    const int64_t d = idx / Lp;
    int64_t j = idx % Lp;
    const float2* st = states + d * T;
    double2 v;
    if (j < T) {
        const float2 q = st[j];
        v = make_double2((double)q.x, (double)q.y);
    } else {
        j -= T;
        const int64_t k = j / A, r = j % A;
        const double* g = noise + (d * n_aug + k) * D;
        if (r == A - 1) {
            const float2 q = st[T - 1];
            v = make_double2((double)q.x + g[D - 4], (double)q.y + g[D - 3]);
        } else {
            const int64_t i = r / per, sub = r % per;
            const float2 cur = st[i];
            double bx = cur.x, by = cur.y;
            if (sub < steps) {
                const float2 nxt = st[i + 1];
                const float f = (float)((double)(sub + 1) / (double)(steps + 1));
                const float dx = nxt.x - cur.x, dy = nxt.y - cur.y;
                const float tx = f * dx, ty = f * dy;
                bx = (double)(cur.x + tx);
                by = (double)(cur.y + ty);
            }
            const double* gn = g + (i * per + sub) * 4;
            v = make_double2(bx + gn[0], by + gn[1]);
        }
    }
    out[idx] = v;
}

// environment.py:166-171: the E best paths (np.argsort ascending, last E), their float32 action
// mean and std over the elites in that order (numpy's float32 reductions: sequential sums, / E,
// sqrt); best [n] = argmax of the rewards (first maximum, environment.py:173). Tied rewards follow
// ascending reward, then path index: numpy's default argsort promises no order for exact ties, so
// this rule is the project's definition there. It decides elite membership and the float32
// summation order, and is pinned by tests/test_gpu_cem_kernels.py (planted ties, a fully tied
// plan) against tests/cem_ref.py, itself held to np.argsort(kind="stable") and the golden
// demonstrations by tests/test_cem_ref_cpu.py. Workgroup = problem; P <= kBlock.
__global__ __launch_bounds__(kBlock) void k_cem_elite(int32_t P, int32_t T, int32_t E,
                                                      const double* __restrict__ reward,
                                                      const float* __restrict__ actions,
                                                      float* __restrict__ mean,
                                                      float* __restrict__ stdv,
                                                      int32_t* __restrict__ best) {
    __shared__ double r[kBlock];
    __shared__ int order[kBlock];
    const int prob = blockIdx.x, tid = threadIdx.x;
    if (tid < P) r[tid] = reward[(int64_t)prob * P + tid];
    __syncthreads();
    if (tid < P) {
        const double v = r[tid];
        int rank = 0;
        for (int q = 0; q < P; ++q) rank += (r[q] < v || (r[q] == v && q < tid)) ? 1 : 0;
        order[rank] = tid;
    }
    __syncthreads();
    if (best && tid == 0) {
        int b = 0;
        for (int q = 1; q < P; ++q)
            if (r[q] > r[b]) b = q;
        best[prob] = b;
    }
    const float* acts = actions + (int64_t)prob * P * T * 2;
    const float inv_n = (float)E;
    for (int k = tid; k < T * 2; k += kBlock) {
        float sum = acts[(int64_t)order[P - E] * T * 2 + k];
        for (int e = 1; e < E; ++e) sum = sum + acts[(int64_t)order[P - E + e] * T * 2 + k];
        const float mu = sum / inv_n;
        float d0 = acts[(int64_t)order[P - E] * T * 2 + k] - mu;
        float sq = d0 * d0;
        for (int e = 1; e < E; ++e) {
            const float d = acts[(int64_t)order[P - E + e] * T * 2 + k] - mu;
            sq = sq + d * d;
        }
        mean[(int64_t)prob * T * 2 + k] = mu;
        stdv[(int64_t)prob * T * 2 + k] = sqrtf(sq / inv_n);
    }
}

}  // namespace

extern "C" {

int nav_rollout(const float* field, int64_t P, int32_t T, const double* start,
                const double* actions, double* paths, const double* goal, double* reward,
                void* stream) {
    if (P < 0 || T < 0 || (P && (!field || !start || !actions || !paths)) || (reward && !goal))
        return NAV_EINVAL;
    if (P == 0) return 0;
    return launch_items(k_rollout, P, stream, f2(field), P, T, d2(start), d2(actions), d2(paths),
                        goal, reward);
}

int nav_cem_rollout(const float* field, int32_t n_prob, int32_t P, int32_t T, int32_t iter,
                    const double* region, const double* uniforms, const double* goal,
                    const double* a0, const double* z, const float* mean, const float* stdv,
                    float* actions, float* paths, double* reward, void* stream) {
    if (!field || n_prob < 0 || P < 1 || T < 1 || iter < 0 || !region || !uniforms || !goal ||
        !actions || !reward || (iter == 0 && !a0) || (iter > 0 && (!z || !mean || !stdv)) ||
        (int64_t)n_prob * P * (T + 1) > ((int64_t)1 << 40))
        return NAV_EINVAL;
    if (n_prob == 0) return 0;
    return launch_items(k_cem_rollout, (int64_t)n_prob * P, stream, f2(field), n_prob, P, T, iter,
                        region, d2(uniforms), d2(goal), d2(a0), d2(z), f2(mean), f2(stdv),
                        f2(actions), f2(paths), reward);
}

int nav_cem_elite(int32_t n_prob, int32_t P, int32_t T, int32_t E, const double* reward,
                  const float* actions, float* mean, float* stdv, int32_t* best, void* stream) {
    if (n_prob < 0 || P < 1 || P > kBlock || T < 1 || E < 1 || E > P || !reward || !actions ||
        !mean || !stdv)
        return NAV_EINVAL;
    if (n_prob == 0) return 0;
    return launch(k_cem_elite, dim3(n_prob), dim3(kBlock), stream, P, T, E, reward, actions, mean,
                  stdv, best);
}

int nav_fields_generate(const double* g5, const double* g10, const double* g20, float* field,
                        void* stream) {
    if (!g5 || !g10 || !g20 || !field) return NAV_EINVAL;
    return launch(k_fields, dim3(1), dim3(kFieldThreads), stream, g5, g10, g20, f2(field));
}

int nav_demo_augment(int32_t n_demo, int32_t T, int32_t steps, int32_t n_aug,
                     const float* states, const double* noise, double* out, void* stream) {
    if (n_demo < 0 || T < 2 || steps < 0 || n_aug < 0 || (n_demo && (!states || !out)) ||
        (n_demo && n_aug && !noise))
        return NAV_EINVAL;
    const int64_t n = (int64_t)n_demo * (T + (int64_t)n_aug * ((int64_t)(T - 1) * (steps + 1) + 1));
    if (n == 0) return 0;
    return launch_items(k_demo_augment, n, stream, n_demo, T, steps, n_aug, f2(states), noise,
                        d2(out));
}

}  // extern "C"
