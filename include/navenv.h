/*
 * navenv.h — C-ABI of libnavenv.so, the MI355X (gfx950) drop-in for the reference's hot path:
 * the Environment.step()/reset() simulator (environment.py) and the residual-TD3 agent's per-step
 * math and learner (robot.py) of benmcclusky/Residual-TD3-Robot-Navigation.
 *
 * Conventions (all entry points):
 *  - plain pointers and sizes only; every array pointer is DEVICE memory owned by the caller
 *    (torch tensors on the Python side), except `nav_params` / `nav_mlp` descriptors, which are
 *    host structs passed by pointer and copied into the launch;
 *  - asynchronous on the given stream (a hipStream_t passed as void*; NULL = default stream);
 *    no allocation, no synchronisation inside a launch function (graph-capturable);
 *  - return 0 on success, NAV_EINVAL for a bad argument (checked on the host before any launch),
 *    or -(hipError_t) when a launch fails; nothing aborts;
 *  - one caller thread per stream; the library keeps no global mutable state;
 *  - outputs and workspaces (learner and acting entry points: the MLP, TD3, glue and tick launches):
 *    a launch writes every element of the extent documented for an output, reads none of them
 *    before it has written it, and stores nowhere else, so no buffer has to be zeroed or otherwise
 *    prepared by the caller. The elements a launch leaves as they were are named at its entry
 *    point: layers whose save-mask bit is clear, columns outside [out_col, out_col + d_out), the
 *    part of an edge slab another launch produces, mask-image row tiles past the last row
 *    workgroup (nav_mlp_mask_count), q_demo rows >= B_demo, ring / cut / pri entries outside the
 *    written window, and any output passed as NULL. Inputs (networks that are only read, the ring,
 *    idx, eps, w, cut) are never written. tests/test_gpu_footprint.py holds every launch to this.
 *
 * Reference interface each entry replaces is cited as file:line of /root/reference.
 */
#ifndef NAVENV_H
#define NAVENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAV_ABI_VERSION 11
#define NAV_EINVAL (-100000)

#define NAV_WORLD_CELLS 100 /* field = float32 [100][100][2] (speed, angle), x-major: cell cx*100+cy
                              (environment.py:20-21 dynamics_speed / dynamics_angle interleaved) */
#define NAV_HIST 5          /* STUCK_STEPS, robot.py:40 */
#define NAV_ROW 8           /* replay row: s0 s1 a0 a1 r s'0 s'1 done (float32) */

/* Philox4x32-10 stream tags (counter word 2). key = (seed_lo, seed_hi). */
#define NAV_TAG_INIT 1   /* ctr = (draw, stream_id, 1, 0)     set_init_and_goal draws   */
#define NAV_TAG_RESET 2  /* ctr = (0, env, 2, episode)        reset draw                */
#define NAV_TAG_NOISE 3  /* ctr = (0, env, 3, step)           exploration noise pair    */
#define NAV_TAG_SAMPLE 4 /* ctr = (i, 0, 4, update)           replay sample index       */
#define NAV_TAG_TNOISE 5 /* ctr = (row, 0, 5, update)         target-smoothing noise    */
#define NAV_TAG_TEST 6   /* ctr = (0, env, 6, episode)        test-episode start draw   */
#define NAV_TAG_DEMO 7   /* ctr = (i, 0, 7, update)           demonstration row index   */
#define NAV_TAG_PER 8    /* ctr = (b, 0, 8, 2*update [+1])    prioritised sample draw   */
#define NAV_TAG_DRESET 9 /* ctr = (0, env, 9, episode)  demo-reset coin, demonstration, index */

/* Constants of constants.py / robot.py as a POD (defaults in nav_default_params). */
typedef struct nav_params {
    double world_size;       /* constants.py:6  WORLD_SIZE = 100 */
    double max_action;       /* constants.py:34 ROBOT_MAX_ACTION = 5 */
    double init_region_size; /* constants.py:25 INIT_REGION_SIZE = 25 */
    double goal_threshold;   /* constants.py:50 TEST_DISTANCE_THRESHOLD = 5 (robot.py:744) */
    double goal_reward;      /* robot.py:42 GOAL_REWARD = 50 */
    double stuck_threshold;  /* robot.py:39 STUCK_THRESHOLD = 2 */
    double stuck_penalty;    /* robot.py:41 STUCK_PENALTY = 50 */
    double demo_factor;      /* robot.py:43 DEMO_PROXIMITY_FACTOR = 10 */
    double noise_decay;      /* robot.py:33 NOISE_DECAY = 0.75 */
    int32_t path_length0;    /* robot.py:28 PATH_LENGTH = 50 */
    int32_t path_increase;   /* robot.py:29 PATH_INCREASE = 20 */
    uint32_t seed_lo, seed_hi; /* configuration.py:26 RANDOM_SEED by default */
    int32_t max_goal_draws;  /* cap on environment.py:52's rejection loop (default 65536) */
} nav_params;

/* Per-env state, structure-of-arrays, n envs (device). */
typedef struct nav_env_soa {
    int64_t n;
    double* state;        /* [n][2]  Environment.robot_state (environment.py:17)           */
    double* goal;         /* [n][2]  Environment.goal_state / Robot.goal_state              */
    double* region;       /* [n][4]  Environment.robot_init_region (left,right,bottom,top)  */
    double* hist;         /* [5][n][2] Robot.previous_states ring (robot.py:425, 509-538)   */
    uint32_t* meta;       /* [n] bit0 goal_reached, bit1 stuck_flag, bit2 demo_flag,
                             bits 8-10 history count, bits 12-14 history head              */
    int32_t* plan_index;  /* [n] Robot.plan_index (robot.py:424) — value at the NEXT step   */
    int32_t* path_length; /* [n] Robot.path_length (robot.py:423)                            */
    int32_t* episodes;    /* [n] Robot.num_episodes (robot.py:421)                           */
    double* noise_scale;  /* [n] Robot.current_noise_scale (robot.py:422)                    */
} nav_env_soa;

/* Per-step outputs of nav_agent_step (device, nullable fields noted). */
typedef struct nav_step_out {
    double* next_state;   /* [n][2] next state BEFORE any auto-reset (Environment.step return) */
    double* goal_term;    /* [n] -||s'-goal|| (robot.py:741), consumed by nav_demo_reward      */
    uint8_t* flags;       /* [n] bit0 done, bit1 goal, bit2 stuck, bit3 ended, bit4 demo term  */
    float* block_stats;   /* nullable: [ceil(n/64)][8], row k = envs [64k, 64k+64): sum of the
                             reward pushed to the replay rows, n_done, n_goal, n_stuck, n_ended,
                             0, 0, 0 (one wave's shuffle tree per row: deterministic). The sum
                             is of the final pushed rewards in every launch form: the demo pass
                             of nav_agent_step_indexed / nav_act_tick runs in the same launch;
                             after nav_agent_step with demo_pending, nav_demo_reward(_indexed)
                             given this pointer rewrites the rows of flagged envs             */
} nav_step_out;

/* Replay ring (device): rows [capacity][8] float32 (robot.py:58-124 ReplayBuffer). */
typedef struct nav_replay {
    float* rows;
    int64_t capacity;
} nav_replay;

/* ReLU MLP (robot.py:128-206) in the device layout: one flat fp32 buffer per network,
 * hidden width padded to a multiple of 32 with zeros (exact: relu(0)=0, zero rows/cols add 0):
 *   W0 [hp][d_in], b0 [hp], {Wl [hp][hp], bl [hp]} x (n_hidden-1), Wo [d_out][hp], bo [d_out]
 * plus `packed` = per hidden->hidden layer the fp16 MFMA B-operand images of the forward
 * (B[k][n] = W[n][k]) then of the backward (B[k][n] = W[k][n]; for d_out = 1 the top hidden
 * layer's backward image holds B[k][n] = fl32(Wo[0][k] W[k][n]), the operand of the row
 * backward's bit-operand product, ABI 11) product: per column n an exponent
 * e_n (B's column max |B| 2^e_n in [2^13, 2^14)) and each entry as two fp16 planes hi =
 * fp16(B 2^e_n), lo = fp16(B 2^e_n - hi) (22 significant bits), laid out [plane 2][hp/16][2][hp][8]
 * (entry (p, k/16, (k/8)&1, n, k&7)) followed by int32 e[hp]: hp^2 + hp floats per image; rebuilt
 * after every writer by nav_adam(_multi) / nav_polyak(_multi) / nav_grad_reduce_adam(_polyak) /
 * nav_mlp_pack (one extra launch on the same stream). ABI 10: the image format (ABI 9: three
 * bf16 planes, 1.5 hp^2 floats). */
typedef struct nav_mlp {
    int32_t d_in;       /* 2 actor (robot.py:145), 4 critic (robot.py:185) */
    int32_t d_out;      /* 2 actor, 1 critic */
    int32_t hidden;     /* logical width: 200 reference, 256 perf config */
    int32_t hidden_pad; /* multiple of 32, <= 256 */
    int32_t n_hidden;   /* hidden layers: 3 reference, 2 perf config */
    float* params;      /* flat, nav_mlp_param_count floats */
    float* packed;      /* nav_mlp_packed_count floats (may be NULL only for n_hidden == 1) */
} nav_mlp;

/* ---- version / descriptors ---- */
int nav_abi_version(void);
void nav_default_params(nav_params* p);
int64_t nav_mlp_param_count(int32_t d_in, int32_t d_out, int32_t hidden_pad, int32_t n_hidden);
int64_t nav_mlp_packed_count(int32_t hidden_pad, int32_t n_hidden);
/* float offset of layer l's W and b inside the flat buffer (l = 0 .. n_hidden) */
int nav_mlp_layer_offsets(const nav_mlp* net, int32_t layer, int64_t* w_off, int64_t* b_off);

/* ---- Environment (environment.py) ---- */
/* environment.py:28-56 set_init_and_goal per env, Philox stream_id = env / envs_per_group (so a
 * group shares region and goal); also initialises the Robot fields to their values at the first
 * training step after the demonstration phase (robot.py:443-489 trace: plan_index 5, path 50,
 * episodes 5, noise 1, demo_flag as given) and draws the first reset (environment.py:130-137).
 * draws_out (nullable) [n]: goal draws used, 0 = rejection cap hit. */
int nav_env_init(const nav_params* p, const nav_env_soa* env, int32_t envs_per_group,
                 int32_t demo_flag, int32_t* draws_out, void* stream);
/* environment.py:130-137 Environment.reset: state = low + (high-low)*u for envs with mask != 0
 * (mask NULL = all). u from `uniforms` [n][2] if given (e.g. the numpy stream of robot-learning.py:19,
 * for reference-stream parity) else Philox (NAV_TAG_RESET, episode = episodes[e]). */
int nav_env_reset(const nav_params* p, const nav_env_soa* env, const uint8_t* mask,
                  const double* uniforms, void* stream);
/* environment.py:122-127 Environment.step for n envs: state <- dynamics(state, action) when the
 * result is inside the world. action [n][2] f64. next_state (nullable) receives the result. */
int nav_env_step(const nav_params* p, const nav_env_soa* env, const float* field,
                 const double* action, double* next_state, void* stream);
/* environment.py:122-127 Environment.step applied K times in one launch (the pure-step loop of
 * robot-learning.py's tick without the agent): the state stays in registers; actions [K][n][2] f64;
 * next_states (nullable) [K][n][2] receives each step's committed state. */
int nav_env_step_k(const nav_params* p, const nav_env_soa* env, const float* field,
                   const double* actions, int32_t K, double* next_states, void* stream);
/* environment.py:98-119 Environment.dynamics, pure: out = f(state, action), n pairs. */
int nav_dynamics(const float* field, const double* state, const double* action, double* out,
                 int64_t n, void* stream);

/* ---- Robot per-step (robot.py) ---- */
/* One training tick for every env, fused: Environment.step (environment.py:122-127) ->
 * Robot.process_transition (robot.py:645-675: reward w/o demo term, check_if_stuck, done, push
 * to the replay row (replay_base + e) % capacity) -> next tick's end-of-episode check and
 * Robot.reset + Environment.reset (robot.py:479-506, environment.py:130-137).
 * demo_pending != 0: the caller runs nav_demo_reward(_indexed) next for the envs flagged
 * (flags bit4) — their demo-proximity term and stuck penalty are written then; 0: no demo set
 * exists, so (robot.py:749-751) the reward is the goal term and the stuck penalty is taken here.
 * replay->capacity must be >= n (one slot per env per launch). */
int nav_agent_step(const nav_params* p, const nav_env_soa* env, const float* field,
                   const double* action, const nav_replay* replay,
                   int64_t replay_base, const nav_step_out* out, int32_t demo_pending,
                   void* stream);
/* Robot.process_transition (robot.py:645-675) without the environment step, for callers that
 * step the Environment themselves (the N = 1 drop-in): reward w/o demo term, check_if_stuck,
 * done, replay push; meta/hist updated, plan_index/path_length read (not advanced).
 * demo_pending as nav_agent_step. */
int nav_transition(const nav_params* p, const nav_env_soa* env, const double* state,
                   const double* action, const double* next_state, const nav_replay* replay,
                   int64_t replay_base, const nav_step_out* out, int32_t demo_pending,
                   void* stream);
/* Robot.check_if_stuck (robot.py:509-538) alone: updates the history ring (hist, meta bits
 * 8-14) with `state` [n][2] and writes stuck [n] (0/1). */
int nav_check_if_stuck(const nav_params* p, const nav_env_soa* env, const double* state,
                       uint8_t* stuck, void* stream);
/* robot.py:741-762 demo-proximity term for envs flagged by nav_agent_step:
 * r = (goal_term + demo_factor * -min_j ||s' - d_j||) - stuck_penalty*stuck, written to the
 * replay row. demo_xy [m][2] f64 per group: group g = env / envs_per_group uses
 * demo_xy[demo_off[g] .. demo_off[g+1]) (demo_off NULL = one shared set of m points).
 * block_stats (nullable, nav_step_out's [ceil(n/64)][8] of the nav_agent_step this pass
 * completes): the reward column of every 64-env row holding a flagged env is summed again from
 * the final pushed rewards, so it equals the one-launch forms' column bit for bit. */
int nav_demo_reward(const nav_params* p, int64_t n, const double* next_state,
                    const double* goal_term, const uint8_t* flags, const double* demo_xy,
                    const int64_t* demo_off, int64_t m, int32_t envs_per_group,
                    const nav_replay* replay, int64_t replay_base, double* reward_out,
                    float* block_stats, void* stream);
/* Exact bucketed nearest-demo index (robot.py:753 made sublinear, result bit-identical to the
 * brute force), built in two levels.
 * Level 1, the 100 x 100 dynamics cells over all points of each group: for each (group, cell) the
 * bound U^2 = min_q maxdist^2(q, cell) and the candidate count (plan), an exclusive scan into
 * cell_start [n_groups*10000 + 1] (scan), then ascending group-relative point indices (fill).
 * cell_bound f64 / cell_count i32: [n_groups][10000]; cand: cell_start[last] int32 entries.
 * Level 2, the query index: every dynamics cell split into R x R index cells (R =
 * nav_demo_index_res(), a power of 2; index cell of s = ((int)(s.x*R), (int)(s.y*R)) on a
 * 100R x 100R grid, x-major), each cell's list taken from its level-1 parent's list (subplan),
 * scanned (subscan) and filled (subfill). sub_bound f64 / sub_count i32: [n_groups][(100R)^2];
 * sub_start [n_groups*(100R)^2 + 1]; sub_cand: sub_start[last] int32 entries. The reward entry
 * points below take (sub_start, sub_cand) as their (cell_start, cand). */
int nav_demo_index_plan(const double* demo_xy, const int64_t* demo_off, int32_t n_groups,
                        int64_t m, double* cell_bound, int32_t* cell_count, void* stream);
int nav_demo_index_scan(const int32_t* cell_count, int32_t n_groups, int64_t* cell_start,
                        void* stream);
int nav_demo_index_fill(const double* demo_xy, const int64_t* demo_off, int32_t n_groups,
                        int64_t m, const double* cell_bound, const int64_t* cell_start,
                        int32_t* cand, void* stream);
int32_t nav_demo_index_res(void);
int nav_demo_index_subplan(const double* demo_xy, const int64_t* demo_off, int32_t n_groups,
                           const int64_t* cell_start, const int32_t* cand, double* sub_bound,
                           int32_t* sub_count, void* stream);
int nav_demo_index_subscan(const int32_t* sub_count, int32_t n_groups, int64_t* sub_start,
                           void* stream);
int nav_demo_index_subfill(const double* demo_xy, const int64_t* demo_off, int32_t n_groups,
                           const int64_t* cell_start, const int32_t* cand,
                           const double* sub_bound, const int64_t* sub_start, int32_t* sub_cand,
                           void* stream);
/* nav_demo_reward through the level-2 index (same result, a few instead of 11 355 points per
 * env; block_stats as there).
 * Contract of the indexed entry points (this one, nav_agent_step_indexed, nav_act_tick(_pop)): a
 * state outside the index, i.e. outside [0,100)^2, is answered by brute force over the group's
 * demo_xy[demo_off[g] .. demo_off[g+1]). With demo_off == NULL these entry points carry no m, so
 * that fallback has no point to visit: they then REQUIRE every flagged s' inside [0,100)^2 (the
 * ticks' own next states always are: the dynamics clip to [0, 98.9999]). A caller who cannot
 * guarantee that, such as one handing its own next_state to nav_demo_reward_indexed, passes a
 * shared set as one group: a two-entry demo_off = {0, m} with envs_per_group >= n, and the index
 * built from the same table (its lists equal the demo_off == NULL build's entry for entry). */
int nav_demo_reward_indexed(const nav_params* p, int64_t n, const double* next_state,
                            const double* goal_term, const uint8_t* flags, const double* demo_xy,
                            const int64_t* demo_off, int32_t envs_per_group,
                            const int64_t* cell_start, const int32_t* cand,
                            const nav_replay* replay, int64_t replay_base, double* reward_out,
                            float* block_stats, void* stream);
/* nav_agent_step + nav_demo_reward_indexed in one launch (same results bit for bit): flagged envs
 * get their demo-proximity reward through the index before the replay row is written, so the row
 * is stored once with the final reward. reward_out (nullable) [n] receives the reward of the
 * flagged envs only, as nav_demo_reward_indexed writes it. Replaces the pair of calls the
 * reference makes per step: robot.py:661-675 process_transition -> compute_reward (727-762). */
int nav_agent_step_indexed(const nav_params* p, const nav_env_soa* env, const float* field,
                           const double* action, const nav_replay* replay, int64_t replay_base,
                           const nav_step_out* out, const double* demo_xy,
                           const int64_t* demo_off, int32_t envs_per_group,
                           const int64_t* cell_start, const int32_t* cand, double* reward_out,
                           void* stream);
/* robot.py:753 min_j ||p_i - d_j|| (scipy cdist euclidean, f64) for n points [n][2]. */
int nav_demo_min(const double* points, int64_t n, const double* demo_xy, int64_t m,
                 double* out, void* stream);
/* Pure robot.py:727-762 compute_reward for n next-states, f64 out; goal_hit (nullable) [n]
 * receives the goal_reached side effect (robot.py:745). */
int nav_compute_reward(const nav_params* p, int64_t n, const double* next_state,
                       const double* goal, const double* demo_xy, int64_t m, int32_t demo_flag,
                       double* reward, uint8_t* goal_hit, void* stream);

/* Batched open-loop rollouts of Environment.dynamics (the CEM demonstrator's inner loop,
 * environment.py:151-165): P paths x T steps; start [P][2], actions [P][T][2] f64 ->
 * paths [P][T+1][2] f64; reward (nullable) [P] = -||f32(s_T) - goal|| (environment.py:182-183). */
int nav_rollout(const float* field, int64_t P, int32_t T, const double* start,
                const double* actions, double* paths, const double* goal, double* reward,
                void* stream);
/* The CEM demonstrator batched over n_prob independent problems (environment.py:140-179; one per
 * (group, demonstration)), P paths x T steps each. nav_cem_rollout runs CEM iteration `iter` for
 * every path of every problem: start = region_sample(region[prob], uniforms[prob]) (environment.py:
 * 150, 136), actions a0 [n][P][T][2] (iteration 0, the +-5 np.random.choice draws) or
 * mean[prob][t] + std[prob][t] * z [n][P][T][2] in f64 (np.random.normal's loc + scale * gauss),
 * written as float32 to actions [n][P][T][2] (planning_actions); paths (nullable) [n][P][T+1][2]
 * float32 (planning_paths); reward [n][P] = -||f32(s_T) - goal|| (environment.py:164, 182-183).
 * nav_cem_elite: per problem the E best paths (ascending reward order, ties by path index), their
 * float32 action mean / std [n][T][2] (numpy float32 reductions over the elites in that order);
 * best (nullable) [n] = first argmax of the rewards (environment.py:166-175). P <= 256. */
int nav_cem_rollout(const float* field, int32_t n_prob, int32_t P, int32_t T, int32_t iter,
                    const double* region, const double* uniforms, const double* goal,
                    const double* a0, const double* z, const float* mean, const float* stdv,
                    float* actions, float* paths, double* reward, void* stream);
int nav_cem_elite(int32_t n_prob, int32_t P, int32_t T, int32_t E, const double* reward,
                  const float* actions, float* mean, float* stdv, int32_t* best, void* stream);
/* environment.py:59-95 set_dynamics as nav.fields restates it (perlin_noise is absent: the field
 * values are parity unpinned against the reference): unit gradient tables g5 [6][6][2],
 * g10 [11][11][2], g20 [21][21][2], f64, from the host's seeded draws. The speed cells mix the
 * three octaves (environment.py:72-74); the angle cells are the SAME octave-5 noise (:85 is the
 * function of :62), min-max normalised. field out [100][100][2] float32 (speed, angle) x-major,
 * the table every dynamics kernel reads. Same f32 values as nav.fields.make_fields (angle bit
 * for bit, speed within 4 ulp: numpy's f32 exp). */
int nav_fields_generate(const double* g5, const double* g10, const double* g20, float* field,
                        void* stream);
/* Robot.process_demonstration's demonstration set for n_demo demonstrations (robot.py:694-698,
 * 771-824): per demo its T states [T][2] (f32, the CEM output) followed by n_aug augmentations
 * of (T-1)*(steps+1) + 1 states each, f64 out [n_demo][T + n_aug*((T-1)(steps+1)+1)][2];
 * noise [n_demo][n_aug][(T-1)(steps+1)*4 + 4] = each augmentation's np.random.normal draws in the
 * reference's order. Bit-identical to the numpy restatement nav.demos.demo_set_from. */
int nav_demo_augment(int32_t n_demo, int32_t T, int32_t steps, int32_t n_aug,
                     const float* states, const double* noise, double* out, void* stream);
/* ReplayBuffer.push (robot.py:79-96) of n transitions (f64 in, float32 rows), slots
 * (base + i) % capacity. */
int nav_replay_push(const nav_replay* replay, int64_t base, int64_t n, const double* state,
                    const double* action, const double* reward, const double* next_state,
                    const uint8_t* done, void* stream);

/* ---- Actor / critic MLPs on MFMA (robot.py:128-206) ---- */
/* Action selection, fused: residual = actor(f32(state - goal)) (robot.py:598-624) and the
 * epilogue a = clip(b + residual + noise, +-max_action) (robot.py:541-569). mode 0 = training
 * (noise = noise_scale*max_action*z; z from `noise_z` [n][2] f64 if given, else Philox
 * NAV_TAG_NOISE at `step`), mode 1 = testing (robot.py:572-595, no noise). action_out [n][2] f64;
 * residual_out (nullable) [n][2] f32. */
int nav_act(const nav_params* p, const nav_mlp* actor, int64_t n, const double* state,
            const double* goal, const double* noise_scale, const double* noise_z,
            uint32_t step, int32_t mode, double* action_out, float* residual_out, void* stream);

/* nav_act (training or testing mode, noise from noise_z or Philox) and nav_agent_step_indexed
 * (demo_xy given) / nav_agent_step with demo_pending 0 (demo_xy NULL) in ONE launch: the actor's
 * action epilogue hands each env's action to that env's training tick in the same workgroup, so
 * the action never round-trips through memory (action_out nullable). Same results as the two
 * launches, bit for bit (robot.py:541-569 then the tick of nav_agent_step; the robot-learning.py
 * 'step' tick, robot-learning.py:95-101). */
int nav_act_tick(const nav_params* p, const nav_mlp* actor, const nav_env_soa* env,
                 const float* field, const double* noise_z, uint32_t step, int32_t mode,
                 const nav_replay* replay, int64_t replay_base, const nav_step_out* out,
                 const double* demo_xy, const int64_t* demo_off, int32_t envs_per_group,
                 const int64_t* cell_start, const int32_t* cand, double* action_out,
                 double* reward_out, void* stream);

/* Per-env results of nav_test_rollout (device). */
typedef struct nav_test_out {
    uint8_t* reached;       /* [n] 1 = a step ended within goal_threshold of the goal          */
    int32_t* steps;         /* [n] the 1-based step that reached, else max_steps               */
    double*  best_distance; /* [n] min over the steps taken of ||s - goal|| (the reaching step
                               included; robot-learning.py:113-114)                            */
    double*  final_state;   /* [n][2] state after the last step taken                          */
    double*  traj;          /* nullable [max_steps][n][2]: state after each step; a stopped
                               env's later rows repeat its final state                         */
} nav_test_out;

/* A whole test episode of every env in ONE launch (robot-learning.py:78, 104-117): from its start
 * (`start` [n][2] if given, else region_sample(region[e], u01(w.x, w.y), u01(w.z, w.w)) with w =
 * philox(0, e, NAV_TAG_TEST, episode): Environment.reset's formula on a stream of its own), env e
 * repeats nav_act mode 1 (no noise) and nav_env_step until a step ends within goal_threshold of
 * its goal or max_steps (1 .. 1 << 20) steps are taken. Same states as that two-launch loop, bit
 * for bit. Reads env->goal (and env->region when start is NULL), the field and the actor; writes
 * only `out`: the env SoA, the replay ring and the actor are untouched. */
int nav_test_rollout(const nav_params* p, const nav_mlp* actor, const nav_env_soa* env,
                     const float* field, const double* start, uint32_t episode,
                     int32_t max_steps, const nav_test_out* out, void* stream);

/* ---- Populations: P members with their own actor, constants and replay ring in ONE launch ----
 * env->n = n_members * envs_per_member; member m owns the consecutive envs [m * envs_per_member,
 * (m + 1) * envs_per_member). `params`, `actors` and `replays` are host arrays [n_members].
 * Every entry point below checks on the host, before any HIP call (NAV_EINVAL): n_members in
 * 1 .. 256; envs_per_member a multiple of 64 (a workgroup sees one member) and, when a demo set
 * is given, of envs_per_group; the actors' d_in / d_out / hidden / hidden_pad / n_hidden equal;
 * the members' world_size, init_region_size, seed_lo / seed_hi and max_goal_draws equal (they
 * key the Philox streams and the init); ring capacities equal and >= envs_per_member; no null
 * pointer. Every other field of nav_params may differ per member.
 * `table` is device memory of nav_pop_table_bytes(n_members) bytes that nav_pop_table_build
 * fills on the stream from the same arrays (replays nullable: a table for test rollouts only):
 * the kernels read member m's actor descriptor, constants and ring pointer from it. Build it
 * once per population, not per step, and again only when a descriptor's pointers, a constant
 * or a ring changes (updating the weights in place needs no rebuild). The launch entry points
 * take the host arrays for the check and the launch shape only; a table built from other
 * arrays is the caller's error. */
int64_t nav_pop_table_bytes(int32_t n_members);
int nav_pop_table_build(const nav_params* params, const nav_mlp* actors,
                        const nav_replay* replays, int32_t n_members, int32_t envs_per_member,
                        void* table, void* stream);
/* nav_act_tick for every member in one launch: member m's rows run actors[m] and params[m] and
 * push to ring m; env e of member m writes slot (replay_base + e - m * envs_per_member) %
 * capacity of ring m (one replay_base for all). Exploration noise stays keyed by the global env
 * index and the common seed, demo groups by the global env index. Member m's envs end exactly
 * as after nav_act_tick over the whole env set with actors[m] and params[m], bit for bit. */
int nav_act_tick_pop(const nav_params* params, const nav_mlp* actors, const nav_replay* replays,
                     int32_t n_members, int32_t envs_per_member, const void* table,
                     const nav_env_soa* env, const float* field, const double* noise_z,
                     uint32_t step, int32_t mode, int64_t replay_base, const nav_step_out* out,
                     const double* demo_xy, const int64_t* demo_off, int32_t envs_per_group,
                     const int64_t* cell_start, const int32_t* cand, double* action_out,
                     double* reward_out, void* stream);
/* nav_test_rollout for every member in one launch: member m's envs run actors[m] with
 * params[m]'s max_action and goal_threshold; start draws stay keyed by the global env index. */
int nav_test_rollout_pop(const nav_params* params, const nav_mlp* actors, int32_t n_members,
                         int32_t envs_per_member, const void* table, const nav_env_soa* env,
                         const float* field, const double* start, uint32_t episode,
                         int32_t max_steps, const nav_test_out* out, void* stream);
/* Per-member scores of a population test rollout (device, [n_members]): what a population-based
 * training step ranks the members by. */
typedef struct nav_pop_score {
    int64_t reached;        /* envs of the member with reached != 0            */
    int64_t steps_reached;  /* sum of steps over those envs                    */
    double  sum_best;       /* sum of best_distance over the member's envs     */
    double  max_best;       /* max of best_distance over the member's envs     */
} nav_pop_score;
/* Reduces out->reached, steps and best_distance [n_members * envs_per_member], as
 * nav_test_rollout_pop wrote them, to scores [n_members] in one launch: one workgroup per member,
 * a strided per-thread partial, then a fixed tree; no floating-point atomics. The order of a
 * member's sum depends on envs_per_member alone: two calls on the same input give the same bits,
 * member m's score does not depend on n_members, the integer fields are exact. Host checks
 * (NAV_EINVAL): n_members in 1 .. 256, envs_per_member >= 1 and a multiple of 64, none of the
 * three inputs or `scores` null. */
int nav_pop_test_summary(const nav_test_out* out, int32_t n_members, int32_t envs_per_member,
                         nav_pop_score* scores, void* stream);

/* Generic forward of up to 2 networks sharing one input (twin critics), rows [M]:
 * x = in[m*ld_in + in_col + 0..d_in) (f32). out_mode 0: out[m*ld_out + out_col + j] = y;
 * out_mode 1 (target policy smoothing, robot.py:336-339): out = clamp(y + clamp(policy_noise*eps,
 * +-noise_clip), +-max_action) with eps from `eps` [M][2] f32 if given else Philox
 * (NAV_TAG_TNOISE, counter). acts (nullable, per net): [n_hidden][M][hp] post-ReLU activations,
 * layer L written when bit L of save_mask is set (rows [0, M) of that layer in full, the padded
 * columns as exact zeros; the other layers are not touched); masks (nullable, per net):
 * nav_mlp_mask_count u16 words of ReLU-derivative bits (for nav_mlp_backward / nav_mlp_wgrad),
 * written as that function's comment states. out: columns [out_col, out_col + d_out) of rows
 * [0, M) are written, the other columns of an ld_out > d_out row are not touched. */
int nav_mlp_forward(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* in,
                    int32_t ld_in, int32_t in_col, float* const* out, int32_t ld_out,
                    int32_t out_col, int32_t out_mode, const float* eps, float policy_noise,
                    float noise_clip, float max_action, uint32_t seed_lo, uint32_t seed_hi,
                    uint32_t counter, float* const* acts, uint32_t save_mask,
                    uint16_t* const* masks, void* stream);
/* train_critic's row-local part (robot.py:329-353) in one launch: per batch row b, sample
 * rows[k] of the replay ring (k = idx[b] if given, else Philox NAV_TAG_SAMPLE at 2*counter, with
 * replacement over [0, size)) into batch [B][8]; a' = clamp(target_actor(s') + clamp(policy_noise
 * * eps, +-noise_clip), +-max_action) with eps from `eps` [B][2] if given else Philox
 * NAV_TAG_TNOISE at counter; y = r + gamma*min(target_critics[0](s', a'), target_critics[1](s',
 * a'))*(1 - done); then both online critics on (s, a) as nav_td3_critic_forward (dq, loss_part,
 * edge_slabs, acts/save_mask, masks). With row_backward != 0 each online critic's row backward
 * (robot.py:361) follows its forward in the same launch, as nav_mlp_backward of dq with the
 * batch's (s, a) columns as input: W0 / bias partials into edge_slabs, dz rows of dz_save_mask
 * layers into dz[i] (layers without their bit, and all of dz with row_backward == 0, are not
 * touched) — the caller then skips nav_mlp_backward. split_twins: 1 = the twin online
 * critics in separate workgroups (grid.y = 2, each repeating the target passes: the small-batch
 * form), 0 = both in one workgroup, < 0 = the library's choice (split for B <= 2048); the
 * results are bit-identical either way. */
int nav_td3_critic_rows(const nav_mlp* target_actor, const nav_mlp* target_critics,
                        const nav_mlp* critics, const nav_replay* replay, int64_t size,
                        int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                        uint32_t counter, const float* eps, float policy_noise,
                        float noise_clip, float max_action, float gamma, float* batch,
                        float* const* dq, float* const* loss_part, float* const* edge_slabs,
                        float* const* acts, uint32_t save_mask, uint16_t* const* masks,
                        int32_t row_backward, float* const* dz, uint32_t dz_save_mask,
                        int32_t split_twins, void* stream);
/* nav_td3_critic_rows with per-row importance weights (prioritised replay): every argument of
 * nav_td3_critic_rows in order, then w [B] and td_abs (two [B] arrays, both required). With
 * e = q_i - y of row b: dq[i][b] = (e * norm) * w[b], loss_part[i] holds block sums of
 * (e * e) * w[b], td_abs[i][b] = fabsf(e). Everything downstream in the launch reads the
 * weighted dq (the Wo / bo partials, the row backward, and what nav_mlp_wgrad later reads from
 * dq). Both twin forms and row_backward 0 / 1 as the plain form; with w == 1.0f every output the
 * plain form also writes is bit-identical to it. NAV_EINVAL: w or td_abs (or either array) NULL. */
int nav_td3_critic_rows_w(const nav_mlp* target_actor, const nav_mlp* target_critics,
                          const nav_mlp* critics, const nav_replay* replay, int64_t size,
                          int64_t B, const int64_t* idx, uint32_t seed_lo, uint32_t seed_hi,
                          uint32_t counter, const float* eps, float policy_noise,
                          float noise_clip, float max_action, float gamma, float* batch,
                          float* const* dq, float* const* loss_part, float* const* edge_slabs,
                          float* const* acts, uint32_t save_mask, uint16_t* const* masks,
                          int32_t row_backward, float* const* dz, uint32_t dz_save_mask,
                          int32_t split_twins, const float* w, float* const* td_abs,
                          void* stream);
/* train_actor's row-local part (robot.py:382-390) in one launch: sample rows (Philox
 * NAV_TAG_SAMPLE at 2*counter + 1, or idx) into batch [B][8]; actor forward on s (ReLU bits to
 * masks_actor, activations to acts for save_mask bits; the top layer's dWo partials come
 * from registers, so it need not be saved);
 * q [B] (nullable) = critic(s, actor(s)); dL/da of L = -mean(q) through the critic (masks_critic)
 * into da [B][2]; the actor's row backward with dz_save_mask rows to dz and its edge partials. */
int nav_td3_actor_rows(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                       int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                       uint32_t seed_hi, uint32_t counter, float* batch, float* q, float* da,
                       float* acts, uint32_t save_mask, float* dz, uint32_t dz_save_mask,
                       uint16_t* masks_actor, uint16_t* masks_critic, float* edge_slabs,
                       void* stream);
/* nav_td3_actor_rows with a behaviour-cloning term on the batch's first B_demo rows (the
 * demonstration rows, nav_td3_mix_idx's prefix; a_b = the sampled row's own action columns):
 *   L = -q_weight * mean_{b<B} critic(s_b, pi(s_b))
 *       + bc_weight * (1/B_demo) * sum_{b<B_demo} sum_j (pi_j(s_b) - a_{b,j})^2
 * The BC sum runs over the two action components and is averaged over the demonstration rows
 * only (not mse_loss's 1/(2*B_demo)). The critic's dy seed is (float)(-q_weight/B); demonstration
 * rows add (float)(2*bc_weight/B_demo) * (pi_j - a_j) to dL/da_j. da [B][2] holds the total dL/da;
 * bc_part [row blocks] = each block's sum of (pi_j - a_j)^2 over its demonstration rows, added in
 * a fixed order (0 for a block that holds none). critic == NULL is pure BC: no critic pass, q and
 * masks_critic unused (nullable), q_weight ignored, da = the BC gradient alone. With a critic,
 * q_weight = 1, B_demo = 0 and bc_weight = 0 every output equals nav_td3_actor_rows' bit for bit.
 * NAV_EINVAL: B_demo < 0 or > B, bc_weight != 0 with B_demo == 0, bc_part NULL. */
int nav_td3_actor_rows_bc(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                          int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                          uint32_t seed_hi, uint32_t counter, int64_t B_demo, float q_weight,
                          float bc_weight, float* batch, float* q, float* da, float* bc_part,
                          float* acts, uint32_t save_mask, float* dz, uint32_t dz_save_mask,
                          uint16_t* masks_actor, uint16_t* masks_critic, float* edge_slabs,
                          void* stream);
/* nav_td3_actor_rows_bc (with a critic) with the Q-filter of Nair et al. 2018 on its BC term: a
 * demonstration row adds its term only where the critic rates the demonstrated action above the
 * policy's own,
 *   L = -q_weight * mean_{b<B} Q1(s_b, pi(s_b))
 *       + bc_weight * (1/B_demo) * sum_{b<B_demo, keep_b} sum_j (pi_j(s_b) - a_{b,j})^2
 *   keep_b = Q1(s_b, a_b) > Q1(s_b, pi(s_b))   (strict; a NaN compares false: dropped)
 * Q1(s_b, pi(s_b)) is the value written to q[b]; Q1(s_b, a_b) is the same critic, the same weight
 * images, in the same launch, on the sampled row's own action columns: one more critic forward
 * in the workgroups that hold demonstration rows (the batch's prefix). The normaliser stays
 * B_demo, not the number of kept rows, so (float)(2*bc_weight/B_demo) stays a launch constant and
 * no count crosses the workgroups before the backward pass. The decision carries no gradient.
 * q_demo [B] (nullable): Q1(s_b, a_b) of rows b < B_demo; rows >= B_demo are not written.
 * bc_part [row blocks]: each block's sum over its kept rows, in nav_td3_actor_rows_bc's order.
 * keep_part [row blocks]: the block's kept demonstration rows (rows, not row components).
 * With B_demo == 0 every output equals nav_td3_actor_rows_bc's bit for bit, keep_part all 0.
 * NAV_EINVAL: what nav_td3_actor_rows_bc refuses, critic NULL, keep_part NULL, q NULL. */
int nav_td3_actor_rows_bcq(const nav_mlp* actor, const nav_mlp* critic, const nav_replay* replay,
                           int64_t size, int64_t B, const int64_t* idx, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t counter, int64_t B_demo, float q_weight,
                           float bc_weight, float* batch, float* q, float* da, float* bc_part,
                           float* q_demo, int32_t* keep_part, float* acts, uint32_t save_mask,
                           float* dz, uint32_t dz_save_mask, uint16_t* masks_actor,
                           uint16_t* masks_critic, float* edge_slabs, void* stream);
/* u16 words of the ReLU mask image for M rows (layout: [n_hidden][row tiles][hp/32][64], row tile
 * = row / 32, layers strided by T = 4 * ceil(M / 128) row tiles). Every launch that writes masks
 * (nav_mlp_forward, nav_td3_critic_forward, nav_td3_critic_rows(_w), nav_td3_actor_rows(_bc,
 * _bcq) and their population forms) writes, per layer, all [hp/32][64] words of row tiles
 * [0, R * nav_mlp_row_blocks(M)), R = 1 up to 16384 rows and 2 above (a row workgroup's height
 * / 32): that covers every row < M, the rows past M inside a written tile carry the bits of an
 * all-zero input row, and the empty second tile of a last 64-row workgroup is written too. Row
 * tiles from R * nav_mlp_row_blocks(M) up to T are never written and never read. */
int64_t nav_mlp_mask_count(int32_t hidden_pad, int32_t n_hidden, int64_t M);
/* Parameter gradients are produced in two parts that nav_grad_reduce combines:
 *  - edge slabs [row blocks][nav_mlp_edge_count]: per row block of the forward/backward launches
 *    (nav_mlp_row_blocks(M) blocks), partial sums of every parameter except the hidden x hidden
 *    weights, in the flat order with those segments cut out (W0 | b0 .. b_{n_hidden-1} | Wo | bo).
 *    A slab is produced in two parts, each written in full for every block, the last, partial
 *    block included: the output layer's part (Wo | bo and the rounding slots behind bo, as zeros)
 *    and the rest (W0 and every hidden bias, padded units as zeros). nav_td3_critic_forward and
 *    nav_td3_critic_rows(_w) with row_backward == 0 write the output layer's part alone;
 *    nav_mlp_backward writes the rest, and the output layer's part too when h_top is given;
 *    nav_td3_critic_rows(_w) with row_backward != 0 and nav_td3_actor_rows(_bc, _bcq) write both.
 *    nav_grad_reduce* reads every entry of every block, so both parts must have been produced;
 *  - hidden slabs [splits][nav_mlp_hidden_count]: nav_mlp_wgrad's split-M partials of
 *    W_1 .. W_{n_hidden-1}; every entry of every split is written, a split whose rows
 *    [s*P, (s+1)*P) of nav_mlp_wgrad's comment all lie at or past M as zeros (of either sign).
 * Per-block outputs (loss_part, bc_part, keep_part) get one value per row block, every block. */
int64_t nav_mlp_row_blocks(int64_t M);
int64_t nav_mlp_edge_count(int32_t d_in, int32_t d_out, int32_t hidden_pad, int32_t n_hidden);
int64_t nav_mlp_hidden_count(int32_t hidden_pad, int32_t n_hidden);
/* train_critic's online twin forward (robot.py:341-361), nets[2] critics (d_out 1) on
 * x = in[b*ld_in + in_col + 0..4): y = r + gamma*min(q1t, q2t)*(1 - done) from the replay batch
 * [B][8] (r at column 4, done at 7); dq[i] [B] = 2*(q_i - y)/B (mse_loss backward);
 * loss_part[i] [row blocks] = block sums of (q_i - y)^2; edge_slabs[i] (nullable) receive the
 * output layer's Wo / bo partials; acts/save_mask as nav_mlp_forward; masks[i] required. */
int nav_td3_critic_forward(const nav_mlp* nets, int64_t B, const float* in, int32_t ld_in,
                           int32_t in_col, const float* batch, const float* q1t, const float* q2t,
                           float gamma, float* const* dq, float* const* loss_part,
                           float* const* edge_slabs, float* const* acts, uint32_t save_mask,
                           uint16_t* const* masks, void* stream);
/* Row-local backward (autograd of robot.py:355-395) of 1 or 2 networks of the same shape that
 * share the input rows (the twin critics: one launch): per net i, dL/dy rows
 * dy[i][m*ld_dy + 0..d_out) (ld_dy 0: one row for all) and the forward's ReLU masks[i] give dL/dz
 * of every hidden layer, dz_L written to dz[i] [n_hidden][M][hp] for bits L of save_mask (the
 * other layers are not touched); dx[i] (nullable) [M][d_in] = dL/dx.
 * edge_slabs[i] (nullable): per-block W0 / bias partials
 * (input rows from `in`), plus Wo / bo when h_top[i] [M][hp] (top hidden activations) is given.
 * Pointer arrays themselves may be NULL where every entry would be. */
int nav_mlp_backward(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* const* dy,
                     int32_t ld_dy, const uint16_t* const* masks, const float* in, int32_t ld_in,
                     int32_t in_col, const float* const* h_top, float* const* dz,
                     uint32_t save_mask, float* const* dx, float* const* edge_slabs,
                     void* stream);
/* Hidden x hidden weight gradients dW_L = dz_L^T h_{L-1} of 1 or 2 networks (one launch) as
 * `splits` partial slabs slabs[i] [splits][nav_mlp_hidden_count] (rows of split s =
 * [s*P, (s+1)*P), P = ceil(M/splits) rounded up to 32). h_0 is recomputed from `in`,
 * dz_{n_hidden-1} from dy[i] and masks[i]; acts[i] / dz[i] (saved layers 1 .. n_hidden-2) are
 * read only for n_hidden > 2. Any splits >= 1 is valid; nav_mlp_wgrad_splits gives the count
 * that fills the chip (one tile workgroup per CU; for d_out = 1 at n_hidden = 2 the tile is
 * 256 x 32 at hidden_pad 256 and 128 x 64 at hidden_pad 128, else 64 x 64). */
int32_t nav_mlp_wgrad_splits(int32_t n_nets, int32_t d_out, int32_t hidden_pad, int32_t n_hidden,
                             int64_t M);
int nav_mlp_wgrad(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* in,
                  int32_t ld_in, int32_t in_col, const float* const* acts,
                  const float* const* dz, const float* const* dy, int32_t ld_dy,
                  const uint16_t* const* masks, float* const* slabs, int32_t splits,
                  void* stream);
/* grad [param_count] = sum of the hidden slabs (hidden weights) and of the edge slabs (the rest),
 * in a fixed order: all nav_mlp_param_count entries are written, the padded and rounding slots
 * as the sums of the slabs' zeros. The Adam and soft-update forms below write all
 * nav_mlp_param_count entries of params, m, v (and grads, targets) and all nav_mlp_packed_count
 * entries of every packed image they refresh; a padded slot of params, m and v whose gradient
 * slot is zero stays exactly +0.0f. */
int nav_grad_reduce(const nav_mlp* net, const float* hidden_slabs, int32_t splits,
                    const float* edge_slabs, int64_t edge_blocks, float* grad, void* stream);
/* nav_grad_reduce fused with the Adam step (robot.py:236-239, as nav_adam) of 1 or 2 networks in
 * one launch: per net i the reduced gradient (also stored to grads[i] when grads and grads[i]
 * are non-NULL) updates nets[i].params with moments m[i], v[i], step_size[i] =
 * lr/(1-b1^t), bc2_sqrt[i] = sqrt(1-b2^t) (host arrays); refreshes packed. */
int nav_grad_reduce_adam(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs,
                         int32_t splits, const float* const* edge_slabs, int64_t edge_blocks,
                         float* const* grads, float* const* m, float* const* v, float beta1,
                         float beta2, float eps, const float* step_size, const float* bc2_sqrt,
                         void* stream);
/* nav_grad_reduce_adam plus the soft updates of robot.py:283-285 in the same launch: each net's
 * target net_targets[i] <- target*(1-tau) + p_new*tau right after p's Adam step (same thread), and
 * n_pairs (<= 4) further (target, source) pairs whose sources are final (the critics on a policy
 * epoch) by extra blocks; bit-identical to nav_grad_reduce_adam followed by nav_polyak_multi. */
int nav_grad_reduce_adam_polyak(const nav_mlp* nets, int32_t n_nets,
                                const float* const* hidden_slabs, int32_t splits,
                                const float* const* edge_slabs, int64_t edge_blocks,
                                float* const* grads, float* const* m, float* const* v,
                                float beta1, float beta2, float eps, const float* step_size,
                                const float* bc2_sqrt, const nav_mlp* net_targets,
                                const nav_mlp* targets, const nav_mlp* sources, int32_t n_pairs,
                                float tau, void* stream);
/* nav_grad_reduce of 1 or 2 same-shape networks in one launch (the twin critics' gradients into
 * one contiguous bucket for the shared-policy all-reduce). */
int nav_grad_reduce_multi(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs,
                          int32_t splits, const float* const* edge_slabs, int64_t edge_blocks,
                          float* const* grads, void* stream);
/* nav_adam of 1 or 2 networks in one launch on gradients g / grad_div (shared policy, BASELINE
 * config 5: the bucket holds the SUM over ranks after the all-reduce, grad_div = world size, as
 * torch DDP's averaging; grad_div 1 = the plain step, bit-identical to nav_adam). step_size and
 * bc2_sqrt are host arrays [n_nets]. */
int nav_adam_multi(const nav_mlp* nets, int32_t n_nets, const float* const* grads,
                   float* const* m, float* const* v, float beta1, float beta2, float eps,
                   const float* step_size, const float* bc2_sqrt, float grad_div, void* stream);
/* nav_adam_multi + a policy epoch's soft updates (robot.py:283-285) in the same launch: each net's
 * own target net_targets[i] follows its stepped parameters, and the n_pairs (targets[i],
 * sources[i]) pairs (sources not stepped by this call) run beside them — the shared-policy
 * counterpart of nav_grad_reduce_adam_polyak; every written `packed` is rebuilt. */
int nav_adam_polyak_multi(const nav_mlp* nets, int32_t n_nets, const float* const* grads,
                          float* const* m, float* const* v, float beta1, float beta2, float eps,
                          const float* step_size, const float* bc2_sqrt, float grad_div,
                          const nav_mlp* net_targets, const nav_mlp* targets,
                          const nav_mlp* sources, int32_t n_pairs, float tau, void* stream);
/* torch.optim.Adam step (robot.py:236-239; torch 2.10 single-tensor semantics) on a flat buffer,
 * step_size = lr/(1-b1^t), bc2_sqrt = sqrt(1-b2^t) precomputed by the caller; refreshes `packed`
 * of `net` (net->params must equal params). */
int nav_adam(const nav_mlp* net, const float* grad, float* m, float* v, float beta1, float beta2,
             float eps, float step_size, float bc2_sqrt, void* stream);
/* robot.py:293-310 soft update target <- target*(1-tau) + source*tau, refreshing target packed. */
int nav_polyak(const nav_mlp* target, const nav_mlp* source, float tau, void* stream);
/* The same for n <= 4 (target, source) pairs in one launch (TD3.soft_update x 3, robot.py:283-285). */
int nav_polyak_multi(const nav_mlp* targets, const nav_mlp* sources, int32_t n, float tau,
                     void* stream);
/* rebuild `packed` from `params` (after a host-side weight load). */
int nav_mlp_pack(const nav_mlp* net, void* stream);

/* ---- TD3 glue (robot.py:312-398) ---- */
/* ReplayBuffer.sample (robot.py:98-115): batch[b] = rows[idx[b]] with idx from `idx` if given,
 * else uniform with replacement over [0, size) from Philox (NAV_TAG_SAMPLE, counter). */
int nav_replay_sample(const nav_replay* replay, int64_t size, int64_t B, const int64_t* idx,
                      uint32_t seed_lo, uint32_t seed_hi, uint32_t counter, float* batch,
                      void* stream);
/* The sample indices of one epoch with demonstration rows mixed in (one launch, both arrays;
 * either output may be NULL). Rows b >= B_demo get the index the row kernels draw themselves:
 * (w.x * size) >> 32 of Philox NAV_TAG_SAMPLE at 2*counter (idx_critic) and 2*counter + 1
 * (idx_actor). Rows b < B_demo get demo_base + ((w.x * n_demo) >> 32) of Philox NAV_TAG_DEMO,
 * ctr = (b, 0, 7, 2*counter [+ 1]): a row of the demonstration tail behind the ring
 * (demo_base = the ring's capacity) or of a demonstration tensor of its own (demo_base = 0).
 * NAV_EINVAL: B < 1, size < 1, B_demo < 0 or > B, B_demo > 0 with n_demo < 1, demo_base < 0. */
int nav_td3_mix_idx(int64_t size, int64_t B, int64_t B_demo, int64_t demo_base, int64_t n_demo,
                    uint32_t seed_lo, uint32_t seed_hi, uint32_t counter, int64_t* idx_critic,
                    int64_t* idx_actor, void* stream);
/* process_demonstration's transitions (robot.py:704-716) of n_demo demonstrations of T states
 * each as replay rows: row d*(T-1)+i = (s, a, r, s', done) with s = states[d][i],
 * a = actions[d][i], s' = states[d][i+1], done = (i == T-2) and r = compute_reward([s']) before
 * any demonstration is known (robot.py:741-750): gt = -||s' - goal[d]|| formed as the tick forms
 * its goal term (in double from the f32 inputs), r = goal_reward where gt >= -goal_threshold,
 * else gt, rounded once to f32. frame 0 (the learner's frame): the rows as above, the action raw
 * (CEM's unclipped action, as the reference stores it). frame 1 (the acting frame): s <- s - g,
 * s' <- s' - g, a <- clamp(a, +-max_action) - (s - g), each formed in double and rounded once:
 * the residual the actor has to output on its input s - g for the demonstrated, clipped action.
 * NAV_EINVAL: NULL pointers, n_demo < 1, T < 2, frame not 0 or 1. */
int nav_demo_transitions(const nav_params* p, int32_t n_demo, int32_t T, const float* states,
                         const float* actions, const double* goal, int32_t frame, float* rows,
                         void* stream);
/* ---- Prioritised replay (Schaul et al. 2016, the proportional variant) ----
 * One priority per ring row, 32-bit fixed point with 16 fractional bits (65536 = 1.0); every sum
 * is an exact uint64, so a sampled index is a pure function of the stored integers and the Philox
 * words: it does not depend on chunk sizes, the hierarchy's shape or a summation order. */
typedef struct nav_per {
    uint32_t* pri;    /* [capacity] priorities; rows >= size are never read as priorities */
    uint64_t* sums;   /* workspace, nav_per_sums_count(capacity) words (layout private) */
    uint32_t* stat;   /* [4]: [0] running max priority ever written, [1] min over [0,size) at
                         the last nav_per_sums, [2..3] reserved (0) */
    int64_t capacity;
} nav_per;
/* Every entry point below checks on the host, before any HIP call (NAV_EINVAL): a NULL struct or
 * member, capacity < 1, and what each one names. */
/* uint64 words of the `sums` workspace (NAV_EINVAL: capacity < 1). */
int64_t nav_per_sums_count(int64_t capacity);
/* pri = 0, stat = {65536, 0, 0, 0}. */
int nav_per_init(const nav_per* per, void* stream);
/* Rows (pos + i) mod capacity, i < n, receive the current stat[0] (read on the device: no host
 * sync); n = 0 is a no-op. NAV_EINVAL: n < 0 or > capacity, pos outside [0, capacity). */
int nav_per_stamp(const nav_per* per, int64_t pos, int64_t n, void* stream);
/* Rebuild every level of the sum hierarchy, the total S and the minimum (stat[1]) from
 * pri[0..size); rows at or beyond size contribute nothing, whatever their bits hold.
 * NAV_EINVAL: size < 1 or > capacity. */
int nav_per_sums(const nav_per* per, int64_t size, void* stream);
/* One launch, three arrays (any may be NULL, as nav_td3_mix_idx). Row b: r64 = (w.y << 32) | w.x
 * of Philox NAV_TAG_PER at ctr = (b, 0, 8, 2*counter) (idx_actor: 2*counter + 1), t = the high 64
 * bits of r64 * S, idx = min{k : P_k > t} with P_k = sum_{j<=k} pri[j] over [0, size), and
 * w_critic[b] = (float)pow((double)stat[1] / (double)pri[idx_critic[b]], (double)beta): the usual
 * (N p_k / S)^-beta over its maximum, in (0, 1]; exactly 1.0f when all priorities are equal.
 * Needs nav_per_sums since the last write to pri. Draws are independent (not stratified).
 * NAV_EINVAL: size < 1 or > capacity, B < 1, beta < 0 or NaN, w_critic without idx_critic. */
int nav_per_sample(const nav_per* per, int64_t size, int64_t B, uint32_t seed_lo,
                   uint32_t seed_hi, uint32_t counter, float beta, int64_t* idx_critic,
                   float* w_critic, int64_t* idx_actor, void* stream);
/* The new priorities of the sampled rows: for b < B, m = 0.5*((double)|td1[b]| + (double)|td2[b]|)
 * + (double)eps and q = (uint32)clamp(floor(pow(m, (double)alpha) * 65536.0 + 0.5), 1, 2^31 - 1)
 * (NaN gives 1, +inf 2^31 - 1: no stored priority is ever 0). pri[idx[b]] becomes the maximum of
 * q over all b' with idx[b'] == idx[b] (the old value is replaced, not maxed with; deterministic
 * with duplicates), stat[0] = max(stat[0], all q). idx in [0, capacity).
 * NAV_EINVAL: B < 1, NULL idx / td1 / td2, alpha <= 0 or NaN, eps < 0 or NaN. */
int nav_per_update(const nav_per* per, int64_t B, const int64_t* idx, const float* td1,
                   const float* td2, float alpha, float eps, void* stream);
/* ---- Multi-step returns: n-step TD targets from the replay ring ----
 * A tick pushes env e to slot (base + e) % capacity and the ring's write position moves by n_envs
 * per tick, so the successor of ring row k for the same env is row (k + n_envs) % capacity: the
 * stride. Column 7 (done) marks only a path end; the tick also resets an env after a goal or a
 * stuck step, and that lives in nav_step_out.flags bit3 alone. `cut` [capacity] u8 beside the ring
 * keeps it: 1 where the env was reset after that row (a done row is always a cut row). */
/* cut[(pos + i) % capacity] = (flags[i] >> 3) & 1 (nav_step_out.flags bit3 'ended'), i < n;
 * n = 0 is a no-op. NAV_EINVAL: NULL cut / flags, capacity < 1, n < 0 or > capacity,
 * pos outside [0, capacity). */
int nav_nstep_stamp(uint8_t* cut, int64_t capacity, int64_t pos, int64_t n,
                    const uint8_t* flags, void* stream);
#define NAV_NSTEP_MAX 16
/* The critic batch of one epoch as n-step rows. Row b: k0 = idx[b] if idx is given, else the
 * index the row kernels draw themselves ((w.x * size) >> 32 of Philox NAV_TAG_SAMPLE at
 * ctr = (b, 0, 4, 2*counter)). age = (position - 1 - k0) mod capacity (rows written after k0).
 * With k_j = (k0 + j*stride) % capacity, the horizon m is the smallest j >= 1 with
 *   j == n_step, or cut[k_{j-1}] != 0, or (j * stride) > age      (the write head).
 * R = sum_{j<m} g^j * (double)rows[k_j][4] in double, g = (double)gamma, g^j by repeated
 * multiplication, terms added in ascending j (starting from the j = 0 term itself); last =
 * rows[k_{m-1}].
 * staged[b] = { rows[k0][0..3], (float)R, last[5], last[6],
 *               last[7] != 0 ? 1.0f : (float)(1.0 - g^{m-1}) };  steps[b] (nullable) = m.
 * For m == 1 the staged row equals rows[k0] bit for bit. Through nav_td3_critic_rows (or _w) with
 * replay = (staged, capacity B), size = B and idx = 0 .. B-1 the target is the n-step one,
 * y = R + (gamma * min Q'(s_{t+m}, a')) * (1.0f - staged[7]): the effective discount
 * gamma * fl32(1.0f - staged[7]) is exact for m == 1 and within one f32 rounding of gamma^m for
 * m > 1 (0 after a done row).
 * NAV_EINVAL: NULL replay / rows / cut / staged, size < 1 or > capacity, position outside
 * [0, capacity), position != size while size < capacity, stride < 1, n_step < 1 or
 * > NAV_NSTEP_MAX, B < 1, gamma outside [0, 1] or NaN. idx values must lie in [0, size). */
int nav_nstep_rows(const nav_replay* replay, const uint8_t* cut, int64_t size, int64_t position,
                   int64_t stride, int32_t n_step, float gamma, int64_t B, const int64_t* idx,
                   uint32_t seed_lo, uint32_t seed_hi, uint32_t counter, float* staged,
                   int32_t* steps, void* stream);
/* ---- Resets to demonstration states (Nair et al. 2018, "Overcoming Exploration in RL with
 * Demonstrations"): some episodes start on a state of a demonstration ----
 * Runs on the tick's stream after any tick form (nav_agent_step(_indexed), nav_act_tick(_pop)) and
 * works from what the tick left: env e was reset iff flags[e] & 8 (nav_step_out.flags bit3
 * 'ended'), env->episodes[e] is already the new episode's number ep and env->state[e] the
 * init-region draw. For each reset env, with g = e / envs_per_group and
 * w = philox(0, e, NAV_TAG_DRESET, ep) under the key (seed_lo, seed_hi): if u01(w.x, w.y) < p,
 * p = prob_group ? prob_group[g] : prob, then d = (w.z * n_demos) >> 32,
 * t = (w.w * usable[g * n_demos + d]) >> 32 and env->state[e] = (double)demo_states[g * n_demos +
 * d][t]. demo_states [n_groups * n_demos][T][2] f32, group-major (the CEM's states); usable
 * [n_groups * n_demos], each in 1 .. T: the leading states of the demonstration an episode may
 * start on (nav.demos.demo_reset_usable: those outside the goal disc, never the last state).
 * Nothing else of the SoA is written: hist, meta, plan_index, path_length, episodes and
 * noise_scale stay as the tick's own reset left them; envs without bit3 are not touched.
 * prob_group (nullable, device [n_groups], each in [0, 1]) replaces prob per group. counts
 * (nullable, device [ceil(n/64)], cumulative): counts[e / 64] grows by the number of envs of that
 * 64-env row that took a demonstration state (each wave owns its slot: deterministic, no
 * atomics). One env per lane; a lane without bit3 loads its flag byte and nothing else.
 * NAV_EINVAL (on the host, before any HIP call): env, flags, demo_states or usable NULL, n < 0,
 * n_demos < 1, T < 2, envs_per_group < 1, prob outside [0, 1] or NaN; then n == 0 returns 0
 * without a launch; then env->state or env->episodes NULL. */
int nav_demo_reset(const nav_env_soa* env, const uint8_t* flags, uint32_t seed_lo,
                   uint32_t seed_hi, const float* demo_states, const int32_t* usable,
                   int32_t n_demos, int32_t T, int32_t envs_per_group, double prob,
                   const double* prob_group, int64_t* counts, void* stream);
/* Fill / strided copy helpers of the TD3 glue (robot.py:329-339, 386-390). */
int nav_fill(float* x, int64_t n, float value, void* stream);
int nav_strided_copy(const float* src, int32_t ld_src, int32_t col_src, float* dst, int32_t ld_dst,
                     int32_t col_dst, int64_t rows, int32_t cols, void* stream);

/* ---- Population learner: every member's TD3 epoch (robot.py:258-285) in one launch per kernel ----
 * One member: everything its four per-epoch calls (nav_td3_critic_rows, nav_td3_actor_rows,
 * nav_mlp_wgrad, nav_grad_reduce_adam / _polyak) take today. The members share nothing. All
 * pointers are device memory; the workspace is sized for batch B as the single-member calls
 * document it (row blocks = nav_mlp_row_blocks(B)). Nullable: idx_critic, idx_actor and eps (the
 * injected sample indices [B] and smoothing noise [B][2]; NULL = Philox), grad_* (the flat
 * gradients are then not stored), and for n_hidden <= 2 acts* and dz* (no layer is saved). */
typedef struct nav_td3_member {
    nav_mlp actor, critics[2], target_actor, target_critics[2];
    nav_replay replay;
    float *m_actor, *v_actor; /* Adam moments [param_count] */
    float *m_critic[2], *v_critic[2];
    double actor_lr, critic_lr; /* robot.py:236-239 */
    float policy_noise, noise_clip, max_action, gamma, tau;
    uint32_t seed_lo, seed_hi; /* the member's Philox key (sampling, smoothing noise) */
    const int64_t* idx_critic;
    const int64_t* idx_actor;
    const float* eps;
    float* batch;        /* [B][8] the critic phase's sampled rows */
    float* batch_actor;  /* [B][8] the actor phase's */
    float* dq[2];        /* [B] */
    float* loss_part[2]; /* [row blocks] */
    float* edge_slabs[2];    /* [row blocks][nav_mlp_edge_count(4, 1, ..)] */
    float* edge_slabs_actor; /* [row blocks][nav_mlp_edge_count(2, 2, ..)] */
    float* acts[2];          /* [n_hidden][B][hidden_pad] */
    float* acts_actor;
    float* dz[2];
    float* dz_actor;
    uint16_t* masks[2];      /* nav_mlp_mask_count words */
    uint16_t* masks_actor;
    float* q;                /* [B] Q1(s, pi(s)), nullable */
    float* da;               /* [B][2] */
    float* hidden_slabs[2];  /* [max splits][nav_mlp_hidden_count]; the actor uses hidden_slabs[0] */
    float* grad_critic[2];   /* [param_count], nullable */
    float* grad_actor;
} nav_td3_member;
/* `members` is a host array [n_members]; `table` is device memory of
 * nav_td3_pop_table_bytes(n_members) bytes that nav_td3_pop_table_build fills on the stream with
 * every member's kernel arguments for batch B and the given weight-gradient split counts, as
 * nav_pop_table_build does for the tick: once per population, and again only when a pointer, a
 * hyper-parameter, B or a split count changes (the weights, moments and rings change in place
 * without a rebuild). What changes per launch and is common to all members travels by value: the
 * replay fill `size` (the rings have one capacity and advance together), the Philox `counter`,
 * and Adam's betas, eps and bias corrections; so steady-state training copies nothing to the
 * device. Every entry point checks on the host, before any HIP call (NAV_EINVAL): n_members in
 * 1 .. 256, B >= 1, one network shape across members, equal ring capacities, 1 <= size <=
 * capacity, splits >= 1, group in {0, 1}, and every pointer (and save-mask rule) that the
 * single-member entry point refuses. The launches take the host array for the check and the
 * launch shape only; a table built from other arrays is the caller's error. */
int64_t nav_td3_pop_table_bytes(int32_t n_members);
int nav_td3_pop_table_build(const nav_td3_member* members, int32_t n_members, int64_t B,
                            int32_t splits_critic, int32_t splits_actor, void* table,
                            void* stream);
/* nav_td3_critic_rows (robot.py:329-361, row_backward on, the middle layers saved) of every member
 * in one launch: grid (row blocks, twins, members), member m's workgroups read its arguments from
 * the table. split_twins < 0: the library's choice from all members' rows (split for n_members * B
 * <= 2048); the results are bit-identical either way, and equal to member m's own
 * nav_td3_critic_rows with the same size and counter. No L2 warmer rows. */
int nav_td3_critic_rows_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                            const void* table, int64_t size, uint32_t counter,
                            int32_t split_twins, void* stream);
/* nav_td3_actor_rows (robot.py:382-390) of every member in one launch. */
int nav_td3_actor_rows_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                           const void* table, int64_t size, uint32_t counter, void* stream);
/* The split count that fills the chip with all members' tile jobs: 256 / (jobs * n_members), at
 * most one split per 512 rows and at least 1; n_members = 1 gives nav_mlp_wgrad_splits. */
int32_t nav_mlp_wgrad_splits_pop(int32_t n_members, int32_t n_nets, int32_t d_out,
                                 int32_t hidden_pad, int32_t n_hidden, int64_t M);
/* nav_mlp_wgrad of every member in one launch after its rows launch (autograd of
 * robot.py:355-363 / 388-395): group 0 = the twin critics (from batch, dq), group 1 = the actor
 * (from batch_actor, da); `splits` is the group's count the table was built with. Launches
 * nothing for n_hidden == 1. */
int nav_mlp_wgrad_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                      const void* table, int32_t group, int32_t splits, void* stream);
/* nav_grad_reduce_adam of every member's group in one launch (robot.py:236-239), then the packed
 * images of what it wrote in one more. bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) of the
 * common step t; member m's step size is formed on the device as (float)(lr_m / bc1), the two
 * roundings of the host's lr / (1 - b1^t) passed as a float. soft_update != 0 (group 1 only):
 * also the member's three soft updates with its tau (robot.py:283-285), as
 * nav_grad_reduce_adam_polyak. */
int nav_grad_reduce_adam_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                             const void* table, int32_t group, float beta1, float beta2,
                             float eps, double bc1, float bc2_sqrt, int32_t soft_update,
                             void* stream);

/* ---- Population learner with demonstrations: per-member demo mix and BC term ----
 * Beside members[m], what member m's nav_td3_mix_idx and nav_td3_actor_rows_bc calls take: the
 * demonstration prefix of its batches, the rows in the tail behind its ring (at the common ring
 * capacity) and the two weights of the actor's loss. A host array [n_members]. */
typedef struct nav_td3_member_bc {
    int64_t B_demo;        /* rows b < B_demo of both batches are demonstration rows; 0 .. B */
    int64_t n_demo;        /* rows in the tail behind this member's ring */
    float q_weight, bc_weight;
    int64_t* idx_critic;   /* [B], written by the mix launch; must equal members[m].idx_critic */
    int64_t* idx_actor;    /* [B]; must equal members[m].idx_actor */
    float* bc_part;        /* [nav_mlp_row_blocks(B)] */
} nav_td3_member_bc;
/* `bc_table` is device memory of nav_td3_pop_bc_table_bytes(n_members) bytes (n_members times
 * the size for one) that nav_td3_pop_bc_table_build fills on the stream with what the two
 * launches below read: member m's nav_td3_actor_rows_bc arguments (the critic's dy seed
 * (float)(-q_weight/B) and the BC coefficient B_demo ? (float)(2*bc_weight/B_demo) : 0, formed as
 * that entry point forms them) and its mix description. Built as nav_td3_pop_table_build's table:
 * once per population, and again only when a pointer or a hyper-parameter changes; `size` and
 * `counter` travel by value. The table nav_td3_pop_table_build fills is neither read nor changed.
 * Host checks of all three entry points (NAV_EINVAL, before any HIP call): everything
 * nav_td3_actor_rows_pop checks; bc or bc_table NULL; B_demo < 0 or > B; bc_weight != 0 with
 * B_demo == 0; B_demo > 0 with n_demo < 1; bc_part NULL; an idx_* pointer NULL or different from
 * members[m]'s. */
int64_t nav_td3_pop_bc_table_bytes(int32_t n_members);
int nav_td3_pop_bc_table_build(const nav_td3_member* members, const nav_td3_member_bc* bc,
                               int32_t n_members, int64_t B, void* bc_table, void* stream);
/* nav_td3_mix_idx of every member in one launch (grid.y = the member): member m writes its
 * idx_critic and, with actor_too != 0, its idx_actor, from its own seed, B_demo and n_demo with
 * demo_base = the common ring capacity; each array equals member m's own nav_td3_mix_idx call with
 * the same size and counter bit for bit. */
int nav_td3_mix_idx_pop(const nav_td3_member* members, const nav_td3_member_bc* bc,
                        int32_t n_members, int64_t B, const void* bc_table, int64_t size,
                        uint32_t counter, int32_t actor_too, void* stream);
/* nav_td3_actor_rows_bc (with a critic) of every member in one launch: grid (row blocks, 1,
 * members), no L2 warmer rows. Every output of member m equals its own nav_td3_actor_rows_bc with
 * the same size and counter bit for bit, so a member with B_demo = 0, bc_weight = 0 and
 * q_weight = 1 equals nav_td3_actor_rows_pop's output for it. */
int nav_td3_actor_rows_bc_pop(const nav_td3_member* members, const nav_td3_member_bc* bc,
                              int32_t n_members, int64_t B, const void* bc_table, int64_t size,
                              uint32_t counter, void* stream);

/* ---- Population-based training: clone learners inside a population in ONE launch ----
 * For every pair j, member dst[j] receives a byte-for-byte copy of member src[j]'s learner state:
 * `params` of the six networks (actor, critics[2], target_actor, target_critics[2]), their
 * `packed` images (nav_mlp_packed_count floats; none for n_hidden == 1, where `packed` is not
 * looked at), the six Adam moment buffers (m_actor, v_actor, m_critic[2], v_critic[2]) and, if
 * replay_rows > 0, rows [0, replay_rows) of the replay ring (later rows untouched; 0 leaves dst's
 * ring alone). Every other field of nav_td3_member (workspace, seeds, learning rates,
 * hyper-parameters, injected indices) is neither read nor written and may be null.
 * `state_table` is device memory of nav_td3_pop_state_bytes(n_members) bytes (n_members times
 * the size for one, a multiple of 8) that nav_td3_pop_state_build fills on the stream with each
 * member's segment pointers and sizes, from the same array the learner table takes: once per
 * population, and again only when a buffer is replaced. It does not depend on the batch size or
 * the split counts. The pair list travels by value with the launch; the launch allocates, copies
 * and synchronises nothing (graph-capturable): grid (chunk blocks, pairs), a block walks its
 * pair's segments as one range of 16-byte units (every segment is a whole number of them:
 * parameter segments are rounded to 4 floats, hidden_pad is a multiple of 32, ring rows are 32
 * bytes). Host checks (NAV_EINVAL, before any HIP call): n_members in 1 .. 256; n_pairs in
 * 1 .. n_members - 1; every index in [0, n_members); src[j] != dst[j]; no member twice in dst;
 * no member of dst in src (so a launch never reads what it writes; one src may serve several
 * dst); one network shape across members and equal ring capacities; 0 <= replay_rows <=
 * capacity; no null or non-16-byte-aligned segment pointer; state_table not null. */
int64_t nav_td3_pop_state_bytes(int32_t n_members);
int nav_td3_pop_state_build(const nav_td3_member* members, int32_t n_members, void* state_table,
                            void* stream);
int nav_td3_pop_exploit(const nav_td3_member* members, int32_t n_members,
                        const void* state_table, const int32_t* src, const int32_t* dst,
                        int32_t n_pairs, int64_t replay_rows, void* stream);

/* ---- kernel timing (measurement only, not on the reference's interface) ----
 * Timing events recorded with a device-scope release (hipEventReleaseToDevice): bracketing a
 * launch costs no system-scope L2 writeback, so timing the bench's timed region does not stretch
 * it (a default torch/HIP event costs ~6 us of GPU time per record on MI355X). */
int nav_event_create(void** event);
int nav_event_destroy(void* event);
int nav_event_record(void* event, void* stream);
/* waits for `end`, then *ms = end - start */
int nav_event_elapsed_ms(void* start, void* end, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* NAVENV_H */
