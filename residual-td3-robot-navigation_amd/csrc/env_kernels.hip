// env_kernels.hip — the vectorised Environment (environment.py) and the Robot's per-step tick
// (robot.py) as gfx950 kernels: one env per lane, structure-of-arrays state in HBM, f64 state
// math (the reference's robot_state is float64), reward/done counts reduced per block through
// wave shuffles and LDS.
#include <stdlib.h>

#include "env_host.h"

namespace {

NAV_DEV void region_of(int r, double u, double* reg) {
    // environment.py:29-49 (left, right, bottom, top)
    const double W = 100.0, S = 25.0;
    const double v = 0.0 + (W - S - 0.0) * u;
    double l, rr, b, t;
    if (r == 0) { l = 0.0; rr = S; b = v; t = b + S; }
    else if (r == 1) { l = v; rr = l + S; b = W - S; t = W; }
    else if (r == 2) { l = W - S; rr = W; b = v; t = b + S; }
    else { l = v; rr = l + S; b = 0.0; t = S; }
    reg[0] = l; reg[1] = rr; reg[2] = b; reg[3] = t;
}

__global__ __launch_bounds__(kBlock) void k_env_init(nav_params p, nav_env_soa env, int32_t epg,
                                                     int32_t demo_flag, int32_t* draws_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= env.n) return;
    const uint32_t sid = (uint32_t)(e / epg);
    // environment.py:28-56 on the Philox stream (NAV_TAG_INIT, stream id)
    uint4 w = philox(0u, sid, NAV_TAG_INIT, 0u, p.seed_lo, p.seed_hi);
    double reg[4];
    region_of((int)(w.x & 3u), u01(w.z, w.w), reg);
    const double mx = 0.5 * (reg[0] + reg[1]), my = 0.5 * (reg[2] + reg[3]);
    double gx = 0.0, gy = 0.0;
    int32_t used = 0;
    for (int k = 1; k <= p.max_goal_draws; ++k) {
        w = philox((uint32_t)k, sid, NAV_TAG_INIT, 0u, p.seed_lo, p.seed_hi);
        gx = 5.0 + 90.0 * u01(w.x, w.y);
        gy = 5.0 + 90.0 * u01(w.z, w.w);
        if (norm2(gx - mx, gy - my) >= 90.0) { used = k; break; }
    }
    reinterpret_cast<double2*>(env.goal)[e] = make_double2(gx, gy);
    double4* rg = reinterpret_cast<double4*>(env.region);
    rg[e] = make_double4(reg[0], reg[1], reg[2], reg[3]);
    // Robot state at the first training step after 3 demos (robot.py:443-489 trace)
    const int32_t ep0 = 5;
    env.plan_index[e] = 5;
    env.path_length[e] = p.path_length0;
    env.episodes[e] = ep0;
    env.noise_scale[e] = 1.0;  // robot.py:32 INITIAL_NOISE
    env.meta[e] = demo_flag ? M_DEMO : 0u;
    // environment.py:130-137 first reset on the reset stream of this env
    w = philox(0u, (uint32_t)e, NAV_TAG_RESET, (uint32_t)ep0, p.seed_lo, p.seed_hi);
    reinterpret_cast<double2*>(env.state)[e] = region_sample(reg, u01(w.x, w.y), u01(w.z, w.w));
    if (draws_out) draws_out[e] = used;
}

__global__ __launch_bounds__(kBlock) void k_env_reset(nav_params p, nav_env_soa env,
                                                      const uint8_t* mask, const double2* uni) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= env.n) return;
    if (mask && !mask[e]) return;
    double u0, u1;
    if (uni) {
        const double2 u = uni[e];
        u0 = u.x; u1 = u.y;
    } else {
        const uint4 w = philox(0u, (uint32_t)e, NAV_TAG_RESET, (uint32_t)env.episodes[e],
                               p.seed_lo, p.seed_hi);
        u0 = u01(w.x, w.y); u1 = u01(w.z, w.w);
    }
    const double4 r = reinterpret_cast<const double4*>(env.region)[e];
    const double reg[4] = {r.x, r.y, r.z, r.w};
    reinterpret_cast<double2*>(env.state)[e] = region_sample(reg, u0, u1);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void k_env_step(int64_t n, double2* __restrict__ state,
                                                     const float2* __restrict__ field,
                                                     const double2* __restrict__ action,
                                                     double2* __restrict__ next_out) {
    // environment.py:122-127: 16 B state in, 16 B action in, 16 B state out per env
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    double2 s, a;
    if (NT) {
        s.x = __builtin_nontemporal_load(&state[e].x);
        s.y = __builtin_nontemporal_load(&state[e].y);
        a.x = __builtin_nontemporal_load(&action[e].x);
        a.y = __builtin_nontemporal_load(&action[e].y);
    } else {
        s = state[e];
        a = action[e];
    }
    const double2 nx = dynamics(field, s, a);
    const bool ok = in_world(nx);
    if (NT) {
        if (ok) {
            __builtin_nontemporal_store(nx.x, &state[e].x);
            __builtin_nontemporal_store(nx.y, &state[e].y);
        }
    } else if (ok) {
        state[e] = nx;
    }
    if (next_out) next_out[e] = ok ? nx : s;
}

__global__ __launch_bounds__(kBlock) void k_dynamics(int64_t n, const float2* __restrict__ field,
                                                     const double2* __restrict__ s,
                                                     const double2* __restrict__ a,
                                                     double2* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    out[e] = dynamics(field, s[e], a[e]);
}

// Robot.check_if_stuck alone (robot.py:509-538): history ring update + stuck verdict.
__global__ __launch_bounds__(kBlock) void k_check_if_stuck(nav_params p, nav_env_soa env,
                                                           const double2* __restrict__ st,
                                                           uint8_t* __restrict__ stuck_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= env.n) return;
    double2* hist = reinterpret_cast<double2*>(env.hist);
    const double2 s = st[e];
    const uint32_t meta = env.meta[e];
    int cnt = (int)((meta >> 8) & 7u), head = (int)((meta >> 12) & 7u);
    bool stuck = false;
    if (cnt >= NAV_HIST) {
        bool all = true;
        for (int k = 0; k < NAV_HIST; ++k) {
            const double2 h = hist[(int64_t)k * env.n + e];
            all = all && (norm2(s.x - h.x, s.y - h.y) < p.stuck_threshold);
        }
        if (all) {
            stuck = true;
            cnt = 0;
        } else {
            head = head == NAV_HIST - 1 ? 0 : head + 1;
            cnt -= 1;
        }
    }
    int sl = head + cnt;
    if (sl >= NAV_HIST) sl -= NAV_HIST;
    hist[(int64_t)sl * env.n + e] = s;
    cnt += 1;
    env.meta[e] = (meta & 0xffu) | ((uint32_t)cnt << 8) | ((uint32_t)head << 12);
    stuck_out[e] = stuck ? 1 : 0;
}

// Robot.process_transition alone (the N = 1 drop-in's path): s, a, s' given by the caller.
__global__ __launch_bounds__(kBlock) void k_transition(nav_params p, nav_env_soa env,
                                                       const double2* __restrict__ st,
                                                       const double2* __restrict__ act,
                                                       const double2* __restrict__ nst,
                                                       float4* __restrict__ rows, int64_t cap,
                                                       int64_t base, nav_step_out out,
                                                       int32_t demo_pending) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= env.n) return;
    const uint32_t meta = env.meta[e];
    const double2 s = st[e], a = act[e], ns = nst[e];
    const TransOut t = transition(p, env, e, s, a, ns, meta, env.plan_index[e],
                                  env.path_length[e], demo_pending != 0);
    push_row(rows, (base + e) % cap, s, a, t.r, ns, t.done);
    env.meta[e] = t.meta;
    if (out.next_state) reinterpret_cast<double2*>(out.next_state)[e] = nst[e];
    if (out.goal_term) out.goal_term[e] = t.gt;
    if (out.flags) out.flags[e] = flag_byte(t, false);
}

// ReplayBuffer.push (robot.py:79-96) of n transitions given as f64 arrays.
__global__ __launch_bounds__(kBlock) void k_replay_push(int64_t n, const double2* __restrict__ s,
                                                        const double2* __restrict__ a,
                                                        const double* __restrict__ r,
                                                        const double2* __restrict__ s2,
                                                        const uint8_t* __restrict__ d,
                                                        float4* __restrict__ rows, int64_t cap,
                                                        int64_t base) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t slot = (base + i) % cap;
    const double2 x = s[i], y = a[i], z = s2[i];
    rows[2 * slot] = make_float4((float)x.x, (float)x.y, (float)y.x, (float)y.y);
    rows[2 * slot + 1] = make_float4((float)r[i], (float)z.x, (float)z.y, d[i] ? 1.f : 0.f);
}

// One training tick per env (see navenv.h nav_agent_step). DEMO: the demo-proximity reward of
// flagged envs through the index in the same launch (nav_agent_step_indexed): the block's demo
// pass walks all its flagged envs' candidate lists together. One statistics row per wave.
template <bool DEMO>
__global__ __launch_bounds__(kBlock) void k_agent_step(nav_params p, nav_env_soa env,
                                                       const float2* __restrict__ field,
                                                       const double2* __restrict__ action,
                                                       float4* __restrict__ rows, int64_t cap,
                                                       int64_t base, nav_step_out out,
                                                       DemoIdx d, int32_t demo_pending,
                                                       double* __restrict__ reward_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    TickStats st{0.f, 0.f, 0.f, 0.f, 0.f};
    DemoPend pend{false, false, 0.0, make_double2(0.0, 0.0)};
    if (e < env.n)
        st = agent_tick<DEMO>(p, env, field, e, action[e], rows, cap, base, out,
                              demo_pending != 0, pend);
    if (DEMO) {
        __shared__ DemoScratch<kBlock, kBlock> scratch;
        const double r = demo_pass<kBlock, kBlock>(p, d, scratch, pend, e,
                                                   reinterpret_cast<float*>(rows), cap, base,
                                                   reward_out);
        if (pend.need) st.r = (float)r;  // the final reward of a flagged env
    }
    if (out.block_stats && e - (threadIdx.x & 63) < env.n) wave_stats(st, out.block_stats, e);
}

// Environment.step for K consecutive steps per launch (environment.py:122-127 applied K times):
// the state stays in registers, actions [K][n][2] stream in, next_out (nullable) [K][n][2]
// receives every step's committed state. Bytes per env-step 16 (+16 with next_out) + 32/K.
__global__ __launch_bounds__(kBlock) void k_env_step_k(int64_t n, int32_t K,
                                                       double2* __restrict__ state,
                                                       const float2* __restrict__ field,
                                                       const double2* __restrict__ action,
                                                       double2* __restrict__ next_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    double2 s = state[e];
    double2 a = action[e];
    for (int32_t k = 0; k < K; ++k) {
        // the next step's action is in flight under this step's dynamics
        const double2 an = k + 1 < K ? action[(int64_t)(k + 1) * n + e] : a;
        const double2 nx = dynamics(field, s, a);
        if (in_world(nx)) s = nx;
        if (next_out) next_out[(int64_t)k * n + e] = s;
        a = an;
    }
    state[e] = s;
}

__global__ __launch_bounds__(kBlock) void k_compute_reward(nav_params p, int64_t n,
                                                           const double2* __restrict__ ns,
                                                           const double2* __restrict__ goal,
                                                           const double2* __restrict__ demo,
                                                           int64_t m, int32_t demo_flag,
                                                           double* reward, uint8_t* hit) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    const double2 s = ns[e], g = goal[e];
    const double gt = -norm2(s.x - g.x, s.y - g.y);
    double r;
    uint8_t h = 0;
    if (gt >= -p.goal_threshold) {
        r = p.goal_reward;
        h = 1;
    } else if (m == 0) {
        r = gt;
    } else {
        const double mn = sqrt(demo_min_global(demo, m, s.x, s.y));
        r = gt + p.demo_factor * (demo_flag ? -mn : 0.0);
    }
    reward[e] = r;
    if (hit) hit[e] = h;
}

}  // namespace

extern "C" {

int nav_abi_version(void) { return NAV_ABI_VERSION; }

int nav_event_create(void** event) {
    if (!event) return NAV_EINVAL;
    return hip_status(hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(event),
                                              hipEventReleaseToDevice));
}

int nav_event_destroy(void* event) {
    if (!event) return NAV_EINVAL;
    return hip_status(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
}

int nav_event_record(void* event, void* stream) {
    if (!event) return NAV_EINVAL;
    return hip_status(hipEventRecord(reinterpret_cast<hipEvent_t>(event), S(stream)));
}

int nav_event_elapsed_ms(void* start, void* end, float* ms) {
    if (!start || !end || !ms) return NAV_EINVAL;
    hipError_t e = hipEventSynchronize(reinterpret_cast<hipEvent_t>(end));
    if (e == hipSuccess)
        e = hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start),
                                reinterpret_cast<hipEvent_t>(end));
    return hip_status(e);
}

void nav_default_params(nav_params* p) {
    if (!p) return;
    p->world_size = 100.0;
    p->max_action = 5.0;
    p->init_region_size = 25.0;
    p->goal_threshold = 5.0;
    p->goal_reward = 50.0;
    p->stuck_threshold = 2.0;
    p->stuck_penalty = 50.0;
    p->demo_factor = 10.0;
    p->noise_decay = 0.75;
    p->path_length0 = 50;
    p->path_increase = 20;
    p->seed_lo = 1707366464u;
    p->seed_hi = 0u;
    p->max_goal_draws = 1 << 16;
}

int nav_env_init(const nav_params* p, const nav_env_soa* env, int32_t epg, int32_t demo_flag,
                 int32_t* draws_out, void* stream) {
    if (!p || !env_ok(env) || epg <= 0 || p->max_goal_draws <= 0) return NAV_EINVAL;
    if (env->n == 0) return 0;
    return launch_items(k_env_init, env->n, stream, *p, *env, epg, demo_flag, draws_out);
}

int nav_env_reset(const nav_params* p, const nav_env_soa* env, const uint8_t* mask,
                  const double* uniforms, void* stream) {
    // needs state + region; the Philox draw also reads episodes
    if (!p || !env || env->n < 0 ||
        (env->n && (!env->state || !env->region || (!uniforms && !env->episodes))))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    return launch_items(k_env_reset, env->n, stream, *p, *env, mask, d2(uniforms));
}

int nav_env_step(const nav_params* p, const nav_env_soa* env, const float* field,
                 const double* action, double* next_state, void* stream) {
    if (!p || !env || env->n < 0 || !field || (env->n && (!env->state || !action)))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    // Non-temporal state/action streams once the 48 B/env working set is past the 256 MB MALL
    // (>= 4 Mi envs): 219 -> 204 us at 2^24 envs (profiles/r01p_step_ab.log). Below that the
    // state stays cache-resident between steps, so default-policy accesses.
    const bool nt = env->n >= (int64_t(1) << 22);
    return launch_items(nt ? k_env_step<true> : k_env_step<false>, env->n, stream, env->n,
                        d2(env->state), f2(field), d2(action), d2(next_state));
}

int nav_env_step_k(const nav_params* p, const nav_env_soa* env, const float* field,
                   const double* actions, int32_t K, double* next_states, void* stream) {
    if (!p || !env || env->n < 0 || K < 0 || !field ||
        (env->n && K && (!env->state || !actions)))
        return NAV_EINVAL;
    if (env->n == 0 || K == 0) return 0;
    return launch_items(k_env_step_k, env->n, stream, env->n, K, d2(env->state), f2(field),
                        d2(actions), d2(next_states));
}

int nav_dynamics(const float* field, const double* state, const double* action, double* out,
                 int64_t n, void* stream) {
    if (n < 0 || (n && (!field || !state || !action || !out))) return NAV_EINVAL;
    if (n == 0) return 0;
    return launch_items(k_dynamics, n, stream, n, f2(field), d2(state), d2(action), d2(out));
}

int nav_agent_step(const nav_params* p, const nav_env_soa* env, const float* field,
                   const double* action, const nav_replay* replay, int64_t replay_base,
                   const nav_step_out* out, int32_t demo_pending, void* stream) {
    if (!p || !env_ok(env) || !field || !action || !ring_ok(replay, replay_base, env->n) || !out)
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    return launch_items(k_agent_step<false>, env->n, stream, *p, *env, f2(field), d2(action),
                        f4(replay->rows), replay->capacity, ring_origin(replay, replay_base),
                        *out, DemoIdx{}, demo_pending, nullptr);
}

int nav_agent_step_indexed(const nav_params* p, const nav_env_soa* env, const float* field,
                           const double* action, const nav_replay* replay, int64_t replay_base,
                           const nav_step_out* out, const double* demo_xy,
                           const int64_t* demo_off, int32_t envs_per_group,
                           const int64_t* cell_start, const int32_t* cand, double* reward_out,
                           void* stream) {
    if (!p || !env_ok(env) || !field || !action || !ring_ok(replay, replay_base, env->n) ||
        !out || (demo_off && envs_per_group <= 0))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    if (!demo_xy || !cell_start || !cand) return NAV_EINVAL;
    return launch_items(k_agent_step<true>, env->n, stream, *p, *env, f2(field), d2(action),
                        f4(replay->rows), replay->capacity, ring_origin(replay, replay_base),
                        *out, demo_idx(demo_xy, demo_off, envs_per_group, cell_start, cand), 1,
                        reward_out);
}

int nav_transition(const nav_params* p, const nav_env_soa* env, const double* state,
                   const double* action, const double* next_state, const nav_replay* replay,
                   int64_t replay_base, const nav_step_out* out, int32_t demo_pending,
                   void* stream) {
    if (!p || !env || env->n < 0 || !ring_ok(replay, replay_base, env->n) || !out)
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    if (!env->goal || !env->hist || !env->meta || !env->plan_index || !env->path_length ||
        !state || !action || !next_state)
        return NAV_EINVAL;
    return launch_items(k_transition, env->n, stream, *p, *env, d2(state), d2(action),
                        d2(next_state), f4(replay->rows), replay->capacity,
                        ring_origin(replay, replay_base), *out, demo_pending);
}

int nav_check_if_stuck(const nav_params* p, const nav_env_soa* env, const double* state,
                       uint8_t* stuck, void* stream) {
    if (!p || !env || env->n < 0 || (env->n && (!env->hist || !env->meta || !state || !stuck)))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    return launch_items(k_check_if_stuck, env->n, stream, *p, *env, d2(state), stuck);
}

int nav_compute_reward(const nav_params* p, int64_t n, const double* next_state,
                       const double* goal, const double* demo_xy, int64_t m, int32_t demo_flag,
                       double* reward, uint8_t* goal_hit, void* stream) {
    if (!p || n < 0 || m < 0 || (n && (!next_state || !goal || !reward)) || (m && !demo_xy))
        return NAV_EINVAL;
    if (n == 0) return 0;
    return launch_items(k_compute_reward, n, stream, *p, n, d2(next_state), d2(goal),
                        d2(demo_xy), m, demo_flag, reward, goal_hit);
}

int nav_replay_push(const nav_replay* replay, int64_t base, int64_t n, const double* state,
                    const double* action, const double* reward, const double* next_state,
                    const uint8_t* done, void* stream) {
    if (!ring_ok(replay, base) || n < 0 ||
        (n && (!state || !action || !reward || !next_state || !done)))
        return NAV_EINVAL;
    if (n == 0) return 0;
    return launch_items(k_replay_push, n, stream, n, d2(state), d2(action), reward,
                        d2(next_state), done, f4(replay->rows), replay->capacity,
                        ring_origin(replay, base));
}

}  // extern "C"
