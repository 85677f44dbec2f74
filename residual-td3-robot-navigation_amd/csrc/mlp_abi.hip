// mlp_abi.hip — the C ABI (include/navenv.h) of the row kernels: argument checks, the kernels'
// argument structs (rows_args.h) and the dispatch to the launcher object of the network's width
// and the call's role (mlp_rows_nt.hip, mlp_rows_role.h). No kernel is instantiated here and no
// device text is included: the launch contract is all this object shares with the launchers.
#include "mlp_rows_role.h"
#include "pop_host.h"

// the 7 x 8 launcher objects' dispatchers
#define NAV_ROWS_DECL(role, nt) rows_fn NAV_ROWS_FN(role, nt);
#define NAV_ROWS_DECL_ROLE(role) NAV_ROWS_NTS(NAV_ROWS_DECL, role)
NAV_ROWS_ROLES(NAV_ROWS_DECL_ROLE)

namespace {

// a hidden width the row kernels are built for: 32 .. 256 in steps of 32
bool width_ok(int hp) { return hp >= 32 && hp <= 256 && !(hp & 31); }

// a replay fill the samplers can draw from: 1 .. capacity rows, within the 32-bit draw
bool fill_ok(int64_t size, int64_t capacity) {
    return size >= 1 && size <= capacity && size <= ((int64_t)1 << 32);
}

// (role, hp / 32) -> the launcher object
int rows_dispatch(int hp, int fam, int in_mode, int out_mode, const void* args, int n_nets,
                  int64_t M, hipStream_t st) {
#define NAV_ROWS_ENTRY(role, nt) NAV_ROWS_FN(role, nt),
#define NAV_ROWS_ENTRY_ROLE(role) {NAV_ROWS_NTS(NAV_ROWS_ENTRY, role)},
    static rows_fn* const rows[ROLE_COUNT][8] = {NAV_ROWS_ROLES(NAV_ROWS_ENTRY_ROLE)};
    const int rt = row_tiles_for(
        M, fam == FAM_FWD && (out_mode == OUT_TICK || out_mode == OUT_TICK_POP));
    if (!width_ok(hp)) return NAV_EINVAL;
    const int r =
        rows[rows_role(fam, out_mode)][hp / 32 - 1](fam, rt, in_mode, out_mode, args, n_nets, st);
    if (r) return r;
    NAV_CHECK_LAUNCH();
    return 0;
}

template <int IN_MODE, int OUT_MODE>
int launch_fwd(const FwdArgs& a, int n_nets, hipStream_t st) {
    return rows_dispatch(a.net[0].hp, FAM_FWD, IN_MODE, OUT_MODE, &a, n_nets, a.M, st);
}

int launch_bwd(const BwdArgs& a, int n_nets, hipStream_t st) {
    return rows_dispatch(a.net[0].hp, FAM_BWD, 0, 0, &a, n_nets, a.M, st);
}

// ---- what nav_act_tick / nav_act_tick_pop and nav_test_rollout / nav_test_rollout_pop share ----
// the env arrays a tick reads or writes, and the cell index beside a demo set
bool tick_ptrs_ok(const nav_env_soa* env, const double* demo_xy, const int64_t* cell_start,
                  const int32_t* cand) {
    if (!env->state || !env->goal || !env->region || !env->hist || !env->meta ||
        !env->plan_index || !env->path_length || !env->episodes || !env->noise_scale)
        return false;
    return !demo_xy || (cell_start && cand);
}

void fill_tick(FwdArgs& a, const nav_env_soa* env, const float* field, const double* noise_z,
               uint32_t step, int32_t mode, const nav_step_out* out, const double* demo_xy,
               const int64_t* demo_off, int32_t envs_per_group, const int64_t* cell_start,
               const int32_t* cand, double* action_out, double* reward_out) {
    a.M = env->n;
    a.state = env->state;
    a.goal = env->goal;
    a.noise_scale = env->noise_scale;
    a.noise_z = noise_z;
    a.step = step;
    a.act_mode = mode;
    a.action_out = action_out;
    a.env = *env;
    a.field = reinterpret_cast<const float2*>(field);
    a.sout = *out;
    if (demo_xy)
        a.demo = DemoIdx{reinterpret_cast<const double2*>(demo_xy), demo_off,
                         envs_per_group > 0 ? envs_per_group : 1, cell_start, cand};
    a.reward_out = reward_out;
}

// the env arrays a test rollout reads (region only without given starts) and its outputs
bool test_ptrs_ok(const nav_env_soa* env, const double* start, const nav_test_out* out) {
    return env->goal && (start || env->region) && out->reached && out->steps &&
           out->best_distance && out->final_state;
}

void fill_test(TestArgs& a, const nav_env_soa* env, const float* field, const double* start,
               uint32_t episode, int32_t max_steps, const nav_test_out* out) {
    a.n = env->n;
    a.goal = reinterpret_cast<const double2*>(env->goal);
    a.region = reinterpret_cast<const double4*>(env->region);
    a.start = reinterpret_cast<const double2*>(start);
    a.field = reinterpret_cast<const float2*>(field);
    a.episode = episode;
    a.max_steps = max_steps;
    a.out = *out;
}

// ---- populations (nav_pop_table_build, nav_act_tick_pop, nav_test_rollout_pop) ----
// The host-side argument check the population entry points share (before any HIP call): n_envs =
// n_members * envs_per_member, whole 64-row workgroups and (demo set given) whole demo groups per
// member, one network shape, one set of the constants that key the Philox streams and the init,
// one ring capacity >= envs_per_member (replays nullable: no rings). dev[m] receives member m's
// actor.
int pop_check(const nav_params* params, const nav_mlp* actors, const nav_replay* replays,
              int32_t n_members, int32_t envs_per_member, const void* table, int64_t n_envs,
              bool demo, int32_t envs_per_group, MlpDev* dev) {
    if (!params || !actors || !table || n_members < 1 || n_members > kMaxMembers ||
        envs_per_member < 64 || envs_per_member % 64 != 0 ||
        n_envs != (int64_t)n_members * envs_per_member || n_envs >= ((int64_t)1 << 31))
        return NAV_EINVAL;
    if (demo && (envs_per_group <= 0 || envs_per_member % envs_per_group != 0))
        return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        const nav_mlp& a = actors[m];
        const nav_params& p = params[m];
        if (!make_dev(&a, &dev[m]) || a.d_in != 2 || a.d_out != 2) return NAV_EINVAL;
        if (a.hidden != actors[0].hidden || a.hidden_pad != actors[0].hidden_pad ||
            a.n_hidden != actors[0].n_hidden)
            return NAV_EINVAL;
        if (p.world_size != params[0].world_size ||
            p.init_region_size != params[0].init_region_size ||
            p.seed_lo != params[0].seed_lo || p.seed_hi != params[0].seed_hi ||
            p.max_goal_draws != params[0].max_goal_draws)
            return NAV_EINVAL;
        if (replays && (!replays[m].rows || replays[m].capacity != replays[0].capacity ||
                        replays[m].capacity < envs_per_member))
            return NAV_EINVAL;
    }
    return 0;
}

// nav_td3_critic_rows' argument check and kernel arguments (the population table's too)
int critic_rows_args(const nav_mlp* target_actor, const nav_mlp* target_critics,
                     const nav_mlp* critics, const nav_replay* replay, int64_t size,
                     int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                     uint32_t counter, const float* eps, float policy_noise,
                     float noise_clip, float max_action, float gamma, float* batch,
                     float* const* dq, float* const* loss_part, float* const* edge_slabs,
                     float* const* acts, uint32_t save_mask, uint16_t* const* masks,
                     int32_t row_backward, float* const* dz, uint32_t dz_save_mask,
                     int32_t split_twins, CriticRowsArgs& a) {
    if (row_backward && dz_save_mask && !dz) return NAV_EINVAL;
    if (!target_actor || !target_critics || !critics || !replay || !replay->rows || B < 1 ||
        !fill_ok(size, replay->capacity) || !batch || !dq || !loss_part || !masks ||
        !make_dev(target_actor, &a.actor_t) || target_actor->d_in != 2 || target_actor->d_out != 2)
        return NAV_EINVAL;
    for (int i = 0; i < 2; ++i) {
        if (!make_dev(&target_critics[i], &a.critic_t[i]) || !make_dev(&critics[i], &a.critic[i]) ||
            critics[i].d_in != 4 || critics[i].d_out != 1 || target_critics[i].d_in != 4 ||
            target_critics[i].d_out != 1 || !dq[i] || !loss_part[i] || !masks[i])
            return NAV_EINVAL;
        if (a.critic_t[i].hp != a.actor_t.hp || a.critic[i].hp != a.actor_t.hp ||
            a.critic[i].n_hidden != a.critic[0].n_hidden)
            return NAV_EINVAL;
        a.dq[i] = dq[i];
        a.loss_part[i] = loss_part[i];
        a.eslab[i] = edge_slabs ? edge_slabs[i] : nullptr;
        a.acts[i] = acts ? acts[i] : nullptr;
        if (save_mask && !a.acts[i]) return NAV_EINVAL;
        a.masks[i] = masks[i];
        a.dz[i] = dz ? dz[i] : nullptr;
        if (row_backward && ((dz_save_mask && !a.dz[i]) ||
                             (dz_save_mask >> critics[i].n_hidden)))
            return NAV_EINVAL;
    }
    a.row_backward = row_backward ? 1 : 0;
    a.dz_save_mask = row_backward ? dz_save_mask : 0u;
    // Small batches leave most CUs idle and each workgroup's chain of network passes sets the
    // time: the twin online critics then run in separate workgroups (grid.y = 2), each repeating
    // the sampling, target actor and twin target critics (identical values) — 5 instead of 7
    // passes per workgroup. split_twins < 0 picks that form for B <= 2048 (profiles/r02aq).
    a.split_twins = split_twins < 0 ? (B <= 2048 ? 1 : 0) : (split_twins ? 1 : 0);
    a.B = B;
    a.rows = replay->rows;
    a.rsize = size;
    a.idx = idx;
    a.seed_lo = seed_lo;
    a.seed_hi = seed_hi;
    a.sample_ctr = 2u * counter;  // the actor's batch of the same epoch uses 2*counter + 1
    a.noise_ctr = counter;
    a.eps = eps;
    a.policy_noise = policy_noise;
    a.noise_clip = noise_clip;
    a.max_action = max_action;
    a.gamma = gamma;
    a.norm = (float)(2.0 / (double)B);
    a.batch = batch;
    a.ecount = edge_count(a.critic[0]);
    a.save_mask = save_mask;
    return 0;
}

int actor_rows_args(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                    int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                    uint32_t seed_hi, uint32_t counter, float* batch, float* q, float* da,
                    float* acts, uint32_t save_mask, float* dz, uint32_t dz_save_mask,
                    uint16_t* masks_actor, uint16_t* masks_critic, float* edge_slabs,
                    ActorRowsArgs& a) {
    // (critic NULL: nav_td3_actor_rows_bc's pure-BC call, no critic to check)
    if (!actor || !replay || !replay->rows || B < 1 || !fill_ok(size, replay->capacity) ||
        !batch || !da || (save_mask && !acts) || !masks_actor || !masks_critic || !edge_slabs ||
        !make_dev(actor, &a.actor) || actor->d_in != 2 || actor->d_out != 2 ||
        (save_mask >> actor->n_hidden) || (dz_save_mask && !dz) ||
        (dz_save_mask >> actor->n_hidden))
        return NAV_EINVAL;
    if (critic && (!make_dev(critic, &a.critic) || critic->d_in != 4 || critic->d_out != 1 ||
                   a.actor.hp != a.critic.hp))
        return NAV_EINVAL;
    a.B = B;
    a.rows = replay->rows;
    a.rsize = size;
    a.idx = idx;
    a.seed_lo = seed_lo;
    a.seed_hi = seed_hi;
    a.sample_ctr = 2u * counter + 1u;
    a.dq = (float)(-1.0 / (double)B);
    a.batch = batch;
    a.q = q;
    a.da = da;
    a.acts = acts;
    a.save_mask = save_mask;
    a.dz = dz;
    a.dz_save_mask = dz_save_mask;
    a.masks_a = masks_actor;
    a.masks_c = masks_critic;
    a.eslab = edge_slabs;
    a.ecount = edge_count(a.actor);
    return 0;
}

// The BC term beside the plain arguments `r` (filled, so r.B holds), as nav_td3_actor_rows_bc,
// nav_td3_actor_rows_bcq and the population's BC table form it: what they refuse, then `bc` and,
// with a critic pass, dq = -q_weight / B
int bc_extra_args(int64_t B_demo, float q_weight, float bc_weight, float* bc_part, bool critic,
                  ActorRowsArgs& r, ActorBcExtra& bc) {
    if (B_demo < 0 || B_demo > r.B || (bc_weight != 0.f && B_demo == 0) || !bc_part)
        return NAV_EINVAL;
    if (critic) r.dq = (float)(-(double)q_weight / (double)r.B);
    bc.B_demo = B_demo;
    bc.bc_coef = B_demo > 0 ? (float)(2.0 * (double)bc_weight / (double)B_demo) : 0.f;
    bc.bc_part = bc_part;
    return 0;
}

// ---- the population learner's table and row launches ----
// One member's CriticRowsArgs / ActorRowsArgs as TD3._critic_rows / _actor_rows pass them: the row
// backward on, the middle hidden layers' rows saved for the weight gradients. `size` only has to
// pass the check here (the launches carry the real one); no warmers.
int rows_member_fill(const nav_td3_member& t, int64_t B, CriticRowsArgs& c,
                     ActorRowsArgs& a) {
    const int nh = t.critics[0].n_hidden;
    if (nh < 1 || nh >= kMaxLayers || t.actor.n_hidden != nh) return NAV_EINVAL;
    uint32_t mid = 0;
    for (int l = 1; l < nh - 1; ++l) mid |= 1u << l;
    int rc = critic_rows_args(&t.target_actor, t.target_critics, t.critics, &t.replay, 1, B,
                              t.idx_critic, t.seed_lo, t.seed_hi, 0u, t.eps, t.policy_noise,
                              t.noise_clip, t.max_action, t.gamma, t.batch, t.dq, t.loss_part,
                              t.edge_slabs, t.acts, mid, t.masks, 1, t.dz, mid, 0, c);
    if (rc) return rc;
    if (!t.edge_slabs[0] || !t.edge_slabs[1]) return NAV_EINVAL;  // the reduce reads them
    rc = actor_rows_args(&t.actor, &t.critics[0], &t.replay, 1, B, t.idx_actor, t.seed_lo,
                         t.seed_hi, 0u, t.batch_actor, t.q, t.da, t.acts_actor, mid, t.dz_actor,
                         mid, t.masks_actor, t.masks[0], t.edge_slabs_actor, a);
    return rc;
}

// The host-side check the population learner's row entry points share (before any HIP call);
// crit / act (nullable): [n_members] host entries
int td3_pop_check(const nav_td3_member* members, int32_t n_members, int64_t B,
                  CriticRowsArgs* crit, ActorRowsArgs* act) {
    if (!members_same_shape(members, n_members) || B < 1) return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        const nav_td3_member& t = members[m];
        CriticRowsArgs c{};
        ActorRowsArgs a{};
        const int rc = rows_member_fill(t, B, c, a);
        if (rc) return rc;
        if (crit) crit[m] = c;
        if (act) act[m] = a;
    }
    return 0;
}

// ---- the population's BC table, mix launch and BC actor launch ----
// The host-side check the three entry points share (before any HIP call): td3_pop_check, then per
// member what nav_td3_actor_rows_bc and nav_td3_mix_idx refuse and the index pointers the two
// arrays must agree on. rows / mix (nullable): [n_members] host entries of the table's sections,
// the BC arguments formed exactly as nav_td3_actor_rows_bc forms them.
int td3_pop_bc_check(const nav_td3_member* members, const nav_td3_member_bc* bc,
                     int32_t n_members, int64_t B, const void* table, ActorRowsBcArgs* rows,
                     MixMember* mix) {
    if (!bc || !table || !members_same_shape(members, n_members) || B < 1) return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        const nav_td3_member& t = members[m];
        const nav_td3_member_bc& x = bc[m];
        if ((x.B_demo > 0 && (x.n_demo < 1 || x.n_demo > ((int64_t)1 << 32))) ||
            !x.idx_critic || !x.idx_actor || x.idx_critic != t.idx_critic ||
            x.idx_actor != t.idx_actor)
            return NAV_EINVAL;
        CriticRowsArgs c{};
        ActorRowsBcArgs e{};
        int rc = rows_member_fill(t, B, c, e.r);
        if (!rc) rc = bc_extra_args(x.B_demo, x.q_weight, x.bc_weight, x.bc_part, true, e.r, e.bc);
        if (rc) return rc;
        if (rows) rows[m] = e;
        if (mix) mix[m] = MixMember{x.B_demo, x.n_demo, t.seed_lo, t.seed_hi,
                                    {x.idx_critic, x.idx_actor}};
    }
    return 0;
}

}  // namespace

int64_t navi_rows_pop_entry_bytes() {
    static_assert(sizeof(CriticRowsArgs) % 8 == 0 && sizeof(ActorRowsArgs) % 8 == 0,
                  "the table's sections stay 8-byte aligned");
    return (int64_t)(sizeof(CriticRowsArgs) + sizeof(ActorRowsArgs));
}

extern "C" {

int64_t nav_mlp_param_count(int32_t d_in, int32_t d_out, int32_t hp, int32_t n_hidden) {
    nav_mlp n{d_in, d_out, hp, hp, n_hidden, reinterpret_cast<float*>(16),
              reinterpret_cast<float*>(16)};
    MlpDev d;
    if (!make_dev(&n, &d)) return NAV_EINVAL;
    return d.count;
}

int64_t nav_mlp_packed_count(int32_t hp, int32_t n_hidden) {
    if (!width_ok(hp) || n_hidden < 1) return NAV_EINVAL;
    return (int64_t)(n_hidden - 1) * 2 * split_image_floats(hp);
}

int nav_mlp_layer_offsets(const nav_mlp* net, int32_t layer, int64_t* w_off, int64_t* b_off) {
    MlpDev d;
    if (!make_dev(net, &d) || layer < 0 || layer > net->n_hidden) return NAV_EINVAL;
    if (w_off) *w_off = d.w_off[layer];
    if (b_off) *b_off = d.b_off[layer];
    return 0;
}

int nav_act(const nav_params* p, const nav_mlp* actor, int64_t n, const double* state,
            const double* goal, const double* noise_scale, const double* noise_z, uint32_t step,
            int32_t mode, double* action_out, float* residual_out, void* stream) {
    FwdArgs a{};
    if (!p || !make_dev(actor, &a.net[0]) || actor->d_in != 2 || actor->d_out != 2 || n < 0 ||
        (mode != 0 && mode != 1))
        return NAV_EINVAL;
    if (n == 0) return 0;
    if (!state || !goal || !action_out || (mode == 0 && !noise_scale)) return NAV_EINVAL;
    a.M = n;
    a.state = state;
    a.goal = goal;
    a.noise_scale = noise_scale;
    a.noise_z = noise_z;
    a.step = step;
    a.act_mode = mode;
    a.max_action_d = p->max_action;
    a.action_out = action_out;
    a.out[0] = residual_out;
    a.seed_lo = p->seed_lo;
    a.seed_hi = p->seed_hi;
    return launch_fwd<IN_BASELINE, OUT_ACT>(a, 1, S(stream));
}

int nav_act_tick(const nav_params* p, const nav_mlp* actor, const nav_env_soa* env,
                 const float* field, const double* noise_z, uint32_t step, int32_t mode,
                 const nav_replay* replay, int64_t replay_base, const nav_step_out* out,
                 const double* demo_xy, const int64_t* demo_off, int32_t envs_per_group,
                 const int64_t* cell_start, const int32_t* cand, double* action_out,
                 double* reward_out, void* stream) {
    FwdArgs a{};
    if (!p || !env || !make_dev(actor, &a.net[0]) || actor->d_in != 2 || actor->d_out != 2 ||
        (mode != 0 && mode != 1) || !field || !replay || !replay->rows || !out ||
        env->n < 0 || env->n >= ((int64_t)1 << 31) || replay->capacity < env->n ||
        replay->capacity <= 0 || replay_base < 0 || (demo_off && envs_per_group <= 0))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    if (!tick_ptrs_ok(env, demo_xy, cell_start, cand)) return NAV_EINVAL;
    fill_tick(a, env, field, noise_z, step, mode, out, demo_xy, demo_off, envs_per_group,
              cell_start, cand, action_out, reward_out);
    a.max_action_d = p->max_action;
    a.p = *p;
    a.rows = reinterpret_cast<float4*>(replay->rows);
    a.cap = replay->capacity;
    a.base = replay_base % replay->capacity;
    return launch_fwd<IN_BASELINE, OUT_TICK>(a, 1, S(stream));
}

int nav_test_rollout(const nav_params* p, const nav_mlp* actor, const nav_env_soa* env,
                     const float* field, const double* start, uint32_t episode,
                     int32_t max_steps, const nav_test_out* out, void* stream) {
    TestArgs a{};
    if (!p || !env || !field || !out || !make_dev(actor, &a.net) || actor->d_in != 2 ||
        actor->d_out != 2 || max_steps < 1 || max_steps > (1 << 20) || env->n < 0 ||
        env->n >= ((int64_t)1 << 31))
        return NAV_EINVAL;
    if (env->n == 0) return 0;
    if (!test_ptrs_ok(env, start, out)) return NAV_EINVAL;
    fill_test(a, env, field, start, episode, max_steps, out);
    a.max_action = p->max_action;
    a.goal_threshold = p->goal_threshold;
    a.seed_lo = p->seed_lo;
    a.seed_hi = p->seed_hi;
    return rows_dispatch(a.net.hp, FAM_TEST, 0, 0, &a, 1, a.n, S(stream));
}

int64_t nav_pop_table_bytes(int32_t n_members) {
    if (n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    return (int64_t)n_members * (int64_t)sizeof(PopMember);
}

int nav_pop_table_build(const nav_params* params, const nav_mlp* actors,
                        const nav_replay* replays, int32_t n_members, int32_t envs_per_member,
                        void* table, void* stream) {
    MlpDev dev[kMaxMembers];
    const int r = pop_check(params, actors, replays, n_members, envs_per_member, table,
                            (int64_t)n_members * envs_per_member, false, 0, dev);
    if (r) return r;
    static_assert(sizeof(PopMember) % 4 == 0, "copied as 32-bit words");
    PopMember* host = static_cast<PopMember*>(calloc((size_t)n_members, sizeof(PopMember)));
    if (!host) return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        PopMember& pm = host[m];
        pm.net = dev[m];
        pm.p = params[m];
        if (replays) {
            const int64_t cap = replays[m].capacity;
            pm.rows = reinterpret_cast<float4*>(replays[m].rows);
            pm.base_off = (cap - ((int64_t)m * envs_per_member) % cap) % cap;
        }
    }
    const int rc = navi_table_write(host, nav_pop_table_bytes(n_members), table, S(stream));
    free(host);
    return rc;
}

int nav_act_tick_pop(const nav_params* params, const nav_mlp* actors, const nav_replay* replays,
                     int32_t n_members, int32_t envs_per_member, const void* table,
                     const nav_env_soa* env, const float* field, const double* noise_z,
                     uint32_t step, int32_t mode, int64_t replay_base, const nav_step_out* out,
                     const double* demo_xy, const int64_t* demo_off, int32_t envs_per_group,
                     const int64_t* cell_start, const int32_t* cand, double* action_out,
                     double* reward_out, void* stream) {
    MlpDev dev[kMaxMembers];
    if (!env || !replays || (mode != 0 && mode != 1) || !field || !out || replay_base < 0)
        return NAV_EINVAL;
    const int r = pop_check(params, actors, replays, n_members, envs_per_member, table, env->n,
                            demo_xy != nullptr, envs_per_group, dev);
    if (r) return r;
    if (!tick_ptrs_ok(env, demo_xy, cell_start, cand)) return NAV_EINVAL;
    FwdArgs a{};
    fill_tick(a, env, field, noise_z, step, mode, out, demo_xy, demo_off, envs_per_group,
              cell_start, cand, action_out, reward_out);
    a.net[0] = dev[0];  // the common shape: picks the instantiation
    a.p = params[0];    // the common seed of the noise draws
    a.cap = replays[0].capacity;
    a.base = replay_base % a.cap;
    a.pop = static_cast<const PopMember*>(table);
    a.pop_blocks = envs_per_member / 64;
    return launch_fwd<IN_BASELINE, OUT_TICK_POP>(a, 1, S(stream));
}

int nav_test_rollout_pop(const nav_params* params, const nav_mlp* actors, int32_t n_members,
                         int32_t envs_per_member, const void* table, const nav_env_soa* env,
                         const float* field, const double* start, uint32_t episode,
                         int32_t max_steps, const nav_test_out* out, void* stream) {
    MlpDev dev[kMaxMembers];
    if (!env || !field || !out || max_steps < 1 || max_steps > (1 << 20)) return NAV_EINVAL;
    const int r = pop_check(params, actors, nullptr, n_members, envs_per_member, table, env->n,
                            false, 0, dev);
    if (r) return r;
    if (!test_ptrs_ok(env, start, out)) return NAV_EINVAL;
    TestArgs a{};
    fill_test(a, env, field, start, episode, max_steps, out);
    a.net = dev[0];  // the common shape: picks the instantiation
    a.seed_lo = params[0].seed_lo;
    a.seed_hi = params[0].seed_hi;
    a.pop = static_cast<const PopMember*>(table);
    a.pop_blocks = envs_per_member / (32 * row_tiles_for(a.n, false));
    return rows_dispatch(a.net.hp, FAM_TEST_POP, 0, 0, &a, 1, a.n, S(stream));
}

int nav_mlp_forward(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* in,
                    int32_t ld_in, int32_t in_col, float* const* out, int32_t ld_out,
                    int32_t out_col, int32_t out_mode, const float* eps, float policy_noise,
                    float noise_clip, float max_action, uint32_t seed_lo, uint32_t seed_hi,
                    uint32_t counter, float* const* acts, uint32_t save_mask,
                    uint16_t* const* masks, void* stream) {
    FwdArgs a{};
    if (!nets || n_nets < 1 || n_nets > 2 || M < 0 || !out) return NAV_EINVAL;
    for (int i = 0; i < n_nets; ++i) {
        if (!make_dev(&nets[i], &a.net[i]) || !out[i]) return NAV_EINVAL;
        if (a.net[i].hp != a.net[0].hp || a.net[i].d_in != a.net[0].d_in) return NAV_EINVAL;
        a.out[i] = out[i];
        a.acts[i] = acts ? acts[i] : nullptr;
        a.masks[i] = masks ? masks[i] : nullptr;
    }
    if (M == 0) return 0;
    if (!in || in_col < 0 || in_col + a.net[0].d_in > ld_in || out_col < 0 ||
        out_col + a.net[0].d_out > ld_out)
        return NAV_EINVAL;
    a.M = M;
    a.in = in;
    a.ld_in = ld_in;
    a.in_col = in_col;
    a.ld_out = ld_out;
    a.out_col = out_col;
    a.save_mask = save_mask;
    a.eps = eps;
    a.policy_noise = policy_noise;
    a.noise_clip = noise_clip;
    a.max_action = max_action;
    a.seed_lo = seed_lo;
    a.seed_hi = seed_hi;
    a.counter = counter;
    if (out_mode == 0) return launch_fwd<IN_F32, OUT_F32>(a, n_nets, S(stream));
    if (out_mode == 1) {
        if (a.net[0].d_out != 2) return NAV_EINVAL;
        return launch_fwd<IN_F32, OUT_TARGET>(a, n_nets, S(stream));
    }
    return NAV_EINVAL;
}

int64_t nav_mlp_row_blocks(int64_t M) {
    if (M < 0) return NAV_EINVAL;
    const int64_t tm = (int64_t)row_tiles_for(M, false) * 32;
    return (M + tm - 1) / tm;
}

int64_t nav_mlp_edge_count(int32_t d_in, int32_t d_out, int32_t hidden_pad, int32_t n_hidden) {
    nav_mlp n{d_in, d_out, hidden_pad, hidden_pad, n_hidden, reinterpret_cast<float*>(16),
              reinterpret_cast<float*>(16)};
    MlpDev d;
    if (!make_dev(&n, &d)) return NAV_EINVAL;
    return edge_count(d);
}

int64_t nav_mlp_hidden_count(int32_t hidden_pad, int32_t n_hidden) {
    if (!width_ok(hidden_pad) || n_hidden < 1) return NAV_EINVAL;
    return (int64_t)(n_hidden - 1) * hidden_pad * hidden_pad;
}

int nav_td3_critic_forward(const nav_mlp* nets, int64_t B, const float* in, int32_t ld_in,
                           int32_t in_col, const float* batch, const float* q1t, const float* q2t,
                           float gamma, float* const* dq, float* const* loss_part,
                           float* const* edge_slabs, float* const* acts, uint32_t save_mask,
                           uint16_t* const* masks, void* stream) {
    FwdArgs a{};
    if (!nets || B < 1 || !in || !batch || !q1t || !q2t || !dq || !loss_part || !masks)
        return NAV_EINVAL;
    for (int i = 0; i < 2; ++i) {
        if (!make_dev(&nets[i], &a.net[i]) || nets[i].d_out != 1 || !dq[i] || !loss_part[i] ||
            !masks[i])
            return NAV_EINVAL;
        if (a.net[i].hp != a.net[0].hp || a.net[i].d_in != a.net[0].d_in ||
            a.net[i].n_hidden != a.net[0].n_hidden)
            return NAV_EINVAL;
        a.out[i] = dq[i];  // unused by OUT_LOSS, non-null for uniformity
        a.acts[i] = acts ? acts[i] : nullptr;
        if (save_mask && !a.acts[i]) return NAV_EINVAL;
        a.masks[i] = masks[i];
        a.dq[i] = dq[i];
        a.loss_part[i] = loss_part[i];
        a.eslab[i] = edge_slabs ? edge_slabs[i] : nullptr;
    }
    if (in_col < 0 || in_col + a.net[0].d_in > ld_in) return NAV_EINVAL;
    a.M = B;
    a.in = in;
    a.ld_in = ld_in;
    a.in_col = in_col;
    a.save_mask = save_mask;
    a.batch = batch;
    a.qt[0] = q1t;
    a.qt[1] = q2t;
    a.gamma = gamma;
    a.norm = (float)(2.0 / (double)B);
    a.ecount = edge_count(a.net[0]);
    return launch_fwd<IN_F32, OUT_LOSS>(a, 2, S(stream));
}

int nav_td3_critic_rows(const nav_mlp* target_actor, const nav_mlp* target_critics,
                        const nav_mlp* critics, const nav_replay* replay, int64_t size,
                        int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                        uint32_t counter, const float* eps, float policy_noise,
                        float noise_clip, float max_action, float gamma, float* batch,
                        float* const* dq, float* const* loss_part, float* const* edge_slabs,
                        float* const* acts, uint32_t save_mask, uint16_t* const* masks,
                        int32_t row_backward, float* const* dz, uint32_t dz_save_mask,
                        int32_t split_twins, void* stream) {
    CriticRowsArgs a{};
    const int rc = critic_rows_args(target_actor, target_critics, critics, replay, size, B, idx,
                                    seed_lo, seed_hi, counter, eps, policy_noise, noise_clip,
                                    max_action, gamma, batch, dq, loss_part, edge_slabs, acts,
                                    save_mask, masks, row_backward, dz, dz_save_mask, split_twins,
                                    a);
    if (rc) return rc;
    return rows_dispatch(a.actor_t.hp, FAM_CRITIC, 0, 0, &a, 1, a.B, S(stream));
}

int nav_td3_critic_rows_w(const nav_mlp* target_actor, const nav_mlp* target_critics,
                          const nav_mlp* critics, const nav_replay* replay, int64_t size,
                          int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                          uint32_t counter, const float* eps, float policy_noise,
                          float noise_clip, float max_action, float gamma, float* batch,
                          float* const* dq, float* const* loss_part, float* const* edge_slabs,
                          float* const* acts, uint32_t save_mask, uint16_t* const* masks,
                          int32_t row_backward, float* const* dz, uint32_t dz_save_mask,
                          int32_t split_twins, const float* w, float* const* td_abs,
                          void* stream) {
    CriticRowsWArgs x{};
    if (!w || !td_abs || !td_abs[0] || !td_abs[1]) return NAV_EINVAL;
    const int rc = critic_rows_args(target_actor, target_critics, critics, replay, size, B, idx,
                                    seed_lo, seed_hi, counter, eps, policy_noise, noise_clip,
                                    max_action, gamma, batch, dq, loss_part, edge_slabs, acts,
                                    save_mask, masks, row_backward, dz, dz_save_mask, split_twins,
                                    x.r);
    if (rc) return rc;
    x.per.w = w;
    x.per.td_abs[0] = td_abs[0];
    x.per.td_abs[1] = td_abs[1];
    return rows_dispatch(x.r.actor_t.hp, FAM_CRITIC_W, 0, 0, &x, 1, x.r.B, S(stream));
}

int nav_td3_actor_rows(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                       int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                       uint32_t seed_hi, uint32_t counter, float* batch, float* q, float* da,
                       float* acts, uint32_t save_mask, float* dz, uint32_t dz_save_mask,
                       uint16_t* masks_actor, uint16_t* masks_critic, float* edge_slabs,
                       void* stream) {
    ActorRowsArgs a{};
    if (!critic) return NAV_EINVAL;
    const int rc = actor_rows_args(actor, critic, replay, size, B, idx, seed_lo, seed_hi, counter,
                                   batch, q, da, acts, save_mask, dz, dz_save_mask, masks_actor,
                                   masks_critic, edge_slabs, a);
    if (rc) return rc;
    return rows_dispatch(a.actor.hp, FAM_ACTOR, 0, 0, &a, 1, a.B, S(stream));
}

int nav_td3_actor_rows_bc(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                          int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                          uint32_t seed_hi, uint32_t counter, int64_t B_demo, float q_weight,
                          float bc_weight, float* batch, float* q, float* da, float* bc_part,
                          float* acts, uint32_t save_mask, float* dz, uint32_t dz_save_mask,
                          uint16_t* masks_actor, uint16_t* masks_critic, float* edge_slabs,
                          void* stream) {
    ActorRowsBcArgs x{};
    // pure BC: the plain check with no q and the actor's mask buffer standing in for the critic's
    x.bc_only = critic ? 0 : 1;
    int rc = actor_rows_args(actor, critic, replay, size, B, idx, seed_lo, seed_hi, counter, batch,
                             critic ? q : nullptr, da, acts, save_mask, dz, dz_save_mask,
                             masks_actor, critic ? masks_critic : masks_actor, edge_slabs, x.r);
    if (!rc) rc = bc_extra_args(B_demo, q_weight, bc_weight, bc_part, !x.bc_only, x.r, x.bc);
    if (rc) return rc;
    if (x.bc_only) {
        x.r.critic = x.r.actor;
        x.r.masks_c = nullptr;
    }
    return rows_dispatch(x.r.actor.hp, FAM_ACTOR_BC, 0, 0, &x, 1, x.r.B, S(stream));
}

int nav_td3_actor_rows_bcq(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                           int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t counter, int64_t B_demo, float q_weight,
                           float bc_weight, float* batch, float* q, float* da, float* bc_part,
                           float* q_demo, int32_t* keep_part, float* acts, uint32_t save_mask,
                           float* dz, uint32_t dz_save_mask, uint16_t* masks_actor,
                           uint16_t* masks_critic, float* edge_slabs, void* stream) {
    ActorRowsBcqArgs x{};
    // the filter's own refusals: it compares critic 1's values
    if (!critic || !keep_part || !q) return NAV_EINVAL;
    ActorRowsArgs& r = x.b.r;
    int rc = actor_rows_args(actor, critic, replay, size, B, idx, seed_lo, seed_hi, counter, batch,
                             q, da, acts, save_mask, dz, dz_save_mask, masks_actor, masks_critic,
                             edge_slabs, r);
    if (!rc) rc = bc_extra_args(B_demo, q_weight, bc_weight, bc_part, true, r, x.b.bc);
    if (rc) return rc;
    x.qf.q_demo = q_demo;
    x.qf.keep_part = keep_part;
    return rows_dispatch(r.actor.hp, FAM_ACTOR_BCQ, 0, 0, &x, 1, r.B, S(stream));
}

int64_t nav_td3_pop_table_bytes(int32_t n_members) {
    if (n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    return (int64_t)n_members * (navi_rows_pop_entry_bytes() + navi_learner_pop_entry_bytes());
}

int nav_td3_pop_table_build(const nav_td3_member* members, int32_t n_members, int64_t B,
                            int32_t splits_critic, int32_t splits_actor, void* table,
                            void* stream) {
    if (!table || n_members < 1 || n_members > kMaxMembers || splits_critic < 1 ||
        splits_actor < 1)
        return NAV_EINVAL;
    const int64_t bytes = nav_td3_pop_table_bytes(n_members);
    // the host image: [P] CriticRowsArgs | [P] ActorRowsArgs | [P] cross-row entries
    uint32_t* host = static_cast<uint32_t*>(calloc((size_t)bytes / 4 + 1, 4));
    if (!host) return NAV_EINVAL;
    char* h = reinterpret_cast<char*>(host);
    CriticRowsArgs* crit = reinterpret_cast<CriticRowsArgs*>(h);
    ActorRowsArgs* act = reinterpret_cast<ActorRowsArgs*>(h + (size_t)n_members * sizeof(CriticRowsArgs));
    int rc = td3_pop_check(members, n_members, B, crit, act);
    if (!rc)
        rc = navi_learner_pop_fill(members, n_members, B, splits_critic, splits_actor,
                                   h + (size_t)n_members * navi_rows_pop_entry_bytes());
    if (!rc) rc = navi_table_write(host, bytes, table, S(stream));
    free(host);
    return rc;
}

// the three population row launches; bc: the BC form's members (its table is the BC table)
static int rows_pop_launch(const nav_td3_member* members, const nav_td3_member_bc* bc,
                           int32_t n_members, int64_t B, const void* table, int64_t size,
                           uint32_t counter, int32_t split_twins, int fam, void* stream) {
    if (!table) return NAV_EINVAL;
    const int rc = fam == FAM_ACTOR_BC_POP
        ? td3_pop_bc_check(members, bc, n_members, B, table, nullptr, nullptr)
        : td3_pop_check(members, n_members, B, nullptr, nullptr);
    if (rc) return rc;
    if (!fill_ok(size, members[0].replay.capacity)) return NAV_EINVAL;
    RowsPopLaunch a{};
    const char* t = static_cast<const char*>(table);
    a.k.table = fam == FAM_ACTOR_POP ? t + (size_t)n_members * sizeof(CriticRowsArgs) : t;
    a.k.size = size;
    a.k.counter = counter;
    a.k.split_twins = split_twins;
    a.B = B;
    a.n_hidden = members[0].critics[0].n_hidden;
    a.n_members = n_members;
    return rows_dispatch(members[0].actor.hidden_pad, fam, 0, 0, &a, 1, B, S(stream));
}

int nav_td3_critic_rows_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                            const void* table, int64_t size, uint32_t counter,
                            int32_t split_twins, void* stream) {
    // the twins in separate workgroups while all members' rows leave CUs idle, as
    // nav_td3_critic_rows chooses for one member
    const int tw = split_twins < 0 ? ((int64_t)n_members * B <= 2048 ? 1 : 0) : (split_twins ? 1 : 0);
    return rows_pop_launch(members, nullptr, n_members, B, table, size, counter, tw, FAM_CRITIC_POP,
                           stream);
}

int nav_td3_actor_rows_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                           const void* table, int64_t size, uint32_t counter, void* stream) {
    return rows_pop_launch(members, nullptr, n_members, B, table, size, counter, 0, FAM_ACTOR_POP,
                           stream);
}

int64_t nav_td3_pop_bc_table_bytes(int32_t n_members) {
    static_assert(sizeof(ActorRowsBcArgs) % 8 == 0, "the table's sections stay 8-byte aligned");
    if (n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    return (int64_t)n_members * (int64_t)(sizeof(ActorRowsBcArgs) + sizeof(MixMember));
}

int nav_td3_pop_bc_table_build(const nav_td3_member* members, const nav_td3_member_bc* bc,
                               int32_t n_members, int64_t B, void* bc_table, void* stream) {
    if (!bc_table || n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    const int64_t bytes = nav_td3_pop_bc_table_bytes(n_members);
    // the host image: [P] ActorRowsBcArgs | [P] MixMember
    uint32_t* host = static_cast<uint32_t*>(calloc((size_t)bytes / 4 + 1, 4));
    if (!host) return NAV_EINVAL;
    char* h = reinterpret_cast<char*>(host);
    int rc = td3_pop_bc_check(
        members, bc, n_members, B, bc_table, reinterpret_cast<ActorRowsBcArgs*>(h),
        reinterpret_cast<MixMember*>(h + (size_t)n_members * sizeof(ActorRowsBcArgs)));
    if (!rc) rc = navi_table_write(host, bytes, bc_table, S(stream));
    free(host);
    return rc;
}

int nav_td3_mix_idx_pop(const nav_td3_member* members, const nav_td3_member_bc* bc,
                        int32_t n_members, int64_t B, const void* bc_table, int64_t size,
                        uint32_t counter, int32_t actor_too, void* stream) {
    const int rc = td3_pop_bc_check(members, bc, n_members, B, bc_table, nullptr, nullptr);
    if (rc) return rc;
    if (!fill_ok(size, members[0].replay.capacity)) return NAV_EINVAL;
    return navi_mix_idx_pop_launch(
        static_cast<const char*>(bc_table) + (size_t)n_members * sizeof(ActorRowsBcArgs),
        n_members, B, size, members[0].replay.capacity, counter, actor_too, S(stream));
}

int nav_td3_actor_rows_bc_pop(const nav_td3_member* members, const nav_td3_member_bc* bc,
                              int32_t n_members, int64_t B, const void* bc_table, int64_t size,
                              uint32_t counter, void* stream) {
    return rows_pop_launch(members, bc, n_members, B, bc_table, size, counter, 0, FAM_ACTOR_BC_POP,
                           stream);
}

int64_t nav_mlp_mask_count(int32_t hidden_pad, int32_t n_hidden, int64_t M) {
    if (!width_ok(hidden_pad) || n_hidden < 1 || M < 0) return NAV_EINVAL;
    return (int64_t)n_hidden * mask_rowtiles(M) * (hidden_pad / 32) * 64;
}

int nav_mlp_backward(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* const* dy,
                     int32_t ld_dy, const uint16_t* const* masks, const float* in, int32_t ld_in,
                     int32_t in_col, const float* const* h_top, float* const* dz,
                     uint32_t save_mask, float* const* dx, float* const* edge_slabs,
                     void* stream) {
    BwdArgs a{};
    if (!nets || n_nets < 1 || n_nets > 2 || M < 0 || ld_dy < 0 || !dy || !masks) return NAV_EINVAL;
    bool any_edges = false;
    for (int i = 0; i < n_nets; ++i) {
        if (!make_dev(&nets[i], &a.net[i])) return NAV_EINVAL;
        if (a.net[i].hp != a.net[0].hp || a.net[i].d_in != a.net[0].d_in ||
            a.net[i].n_hidden != a.net[0].n_hidden || a.net[i].d_out != a.net[0].d_out)
            return NAV_EINVAL;
        a.dy[i] = dy[i];
        a.masks[i] = masks[i];
        a.h_top[i] = h_top ? h_top[i] : nullptr;
        a.dz[i] = dz ? dz[i] : nullptr;
        a.dx[i] = dx ? dx[i] : nullptr;
        a.eslab[i] = edge_slabs ? edge_slabs[i] : nullptr;
        if (M > 0 && (!a.dy[i] || !a.masks[i] || (save_mask && !a.dz[i]))) return NAV_EINVAL;
        any_edges = any_edges || a.eslab[i];
    }
    if (M == 0) return 0;
    if ((save_mask >> a.net[0].n_hidden) ||
        (any_edges && (!in || in_col < 0 || in_col + a.net[0].d_in > ld_in)))
        return NAV_EINVAL;
    a.M = M;
    a.ld_dy = ld_dy;
    a.in = in;
    a.ld_in = ld_in;
    a.in_col = in_col;
    a.save_mask = save_mask;
    a.ecount = edge_count(a.net[0]);
    return launch_bwd(a, n_nets, S(stream));
}

}  // extern "C"
