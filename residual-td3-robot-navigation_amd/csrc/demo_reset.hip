// demo_reset.hip — resets to demonstration states (Nair et al. 2018, "Overcoming Exploration in
// RL with Demonstrations", the third part beside the BC term and the Q-filter): after a tick, an
// env the tick reset (flags bit 3) starts its new episode, with probability p, on a state of one
// of its own group's CEM demonstrations instead of the init-region draw (nav_demo_reset).
// One env per lane. The flag byte is loaded first and a lane without bit 3 loads nothing else:
// on a typical tick under 2 % of the lanes go on. Only env.state is written; the tick's own
// reset has already set history, plan_index, path_length, episodes and noise_scale.
// A translation unit of its own: every other object of libnavenv.so compiles from the source it
// had before.
#include "env_host.h"

namespace {

using namespace nav;

struct DemoResetArgs {
    double2* state;           // [n]
    const int32_t* episodes;  // [n] the new episode's number
    const uint8_t* flags;     // [n] bit 3: the tick reset this env
    int64_t n;
    uint32_t s0, s1;
    const float2* demo;       // [n_groups * n_demos][T]
    const int32_t* usable;    // [n_groups * n_demos]
    int32_t n_demos, T, epg;
    double prob;
    const double* prob_group;  // nullable [n_groups]
    int64_t* counts;           // nullable [ceil(n / 64)]
};

__global__ __launch_bounds__(kBlock) void k_demo_reset(DemoResetArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool took = false;
    if (e < a.n && (a.flags[e] & 8u)) {
        const int64_t g = e / a.epg;
        const uint4 w =
            philox(0u, (uint32_t)e, NAV_TAG_DRESET, (uint32_t)a.episodes[e], a.s0, a.s1);
        const double p = a.prob_group ? a.prob_group[g] : a.prob;
        if (u01(w.x, w.y) < p) {
            const int64_t j = g * a.n_demos + __umulhi(w.z, (uint32_t)a.n_demos);
            // the table's contract is 1 .. T; the clamp keeps a broken one inside the demonstration
            int32_t u = a.usable[j];
            u = u < 1 ? 1 : (u > a.T ? a.T : u);
            const float2 s = a.demo[j * a.T + __umulhi(w.w, (uint32_t)u)];
            a.state[e] = make_double2((double)s.x, (double)s.y);
            took = true;
        }
    }
    if (a.counts) {
        // kBlock is a multiple of 64, so a wave is one 64-env row and its lane 0 is env 64k < n
        // wherever some lane of it took a state: each wave owns its slot, no atomics
        const unsigned long long b = __ballot(took);
        if (b != 0 && (threadIdx.x & 63) == 0) a.counts[e >> 6] += (int64_t)__popcll(b);
    }
}

}  // namespace

extern "C" int nav_demo_reset(const nav_env_soa* env, const uint8_t* flags, uint32_t seed_lo,
                              uint32_t seed_hi, const float* demo_states, const int32_t* usable,
                              int32_t n_demos, int32_t T, int32_t envs_per_group, double prob,
                              const double* prob_group, int64_t* counts, void* stream) {
    if (!env || env->n < 0 || env->n >= (int64_t)1 << 31 || !flags || !demo_states || !usable ||
        n_demos < 1 || T < 2 || envs_per_group < 1 || !(prob >= 0.0 && prob <= 1.0))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    if (!env->state || !env->episodes) return NAV_EINVAL;
    DemoResetArgs a;
    a.state = d2(env->state);
    a.episodes = env->episodes;
    a.flags = flags;
    a.n = env->n;
    a.s0 = seed_lo;
    a.s1 = seed_hi;
    a.demo = f2(demo_states);
    a.usable = usable;
    a.n_demos = n_demos;
    a.T = T;
    a.epg = envs_per_group;
    a.prob = prob;
    a.prob_group = prob_group;
    a.counts = counts;
    return launch_items(k_demo_reset, a.n, stream, a);
}
