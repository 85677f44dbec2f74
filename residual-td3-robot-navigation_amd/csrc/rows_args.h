// rows_args.h — the launch contract of the row kernels: what the C ABI's object (mlp_abi.hip), the
// 56 launcher objects (mlp_rows_nt.hip, one per hidden width and role) and the kernels themselves
// must agree on. The argument structs travel between those 57 objects as const void*, so every
// object has to see the same definitions: the family and mode numbers, the argument structs, the
// LDS sizes a launch asks for and a kernel carves up, the L2 warmer list and the row-block height.
// A change here changes every object at once; anything else about the row kernels is device text
// (rows_gemm.h, rows_layers.h, rows_kernels.h, td3_rows.h) and none of it is needed, or seen, by
// the ABI's object. Nothing here runs on the device but the constexpr sizes.
#pragma once
#include "mlp_common.h"
#include "nav_tick.h"


namespace {

// ---- family and mode numbers ----
// The row kernels (forward, row backward, critic_rows, actor_rows) are instantiated per NT in
// their own objects (mlp_rows_nt.hip built with NAV_MLP_PART = NT, see the Makefile) so the heavy
// template instantiations compile in parallel; the C ABI's object (mlp_abi.hip) dispatches to
// them through nav_mlp_rows_<role>_<NT>(). Argument structs travel as const void* (same definitions).
enum {
    FAM_FWD = 0, FAM_BWD = 1, FAM_CRITIC = 2, FAM_ACTOR = 3, FAM_TEST = 4, FAM_TEST_POP = 5,
    FAM_CRITIC_POP = 6, FAM_ACTOR_POP = 7, FAM_ACTOR_BC = 8, FAM_ACTOR_BC_POP = 9, FAM_CRITIC_W = 10,
    FAM_ACTOR_BCQ = 11
};

enum { IN_F32 = 0, IN_BASELINE = 1 };
enum { OUT_F32 = 0, OUT_TARGET = 1, OUT_ACT = 2, OUT_LOSS = 3, OUT_TICK = 4, OUT_TICK_POP = 5 };

// ---- launch helpers (template dispatch on NT = hp / 32 and RT = rows / 32) ----
// Workgroup height: RT = 2 (64 rows, two workgroups per CU so one workgroup's epilogue overlaps
// the other's MFMA loop; RT = 4, 128 rows and one workgroup per CU, measured slower in round 1:
// profiles/r01c_micro_rt4.json, no longer built).
// Small batches take RT = 1 (32-row workgroups): at M <= kSmallRows the 64-row grid leaves CUs
// idle (config 1's 100 rows: 2 workgroups), and a 32-row block halves each wave's MFMA chain per
// layer, so the latency-bound small-batch learner runs twice the workgroups at half the chain.
// Not for the fused tick (its demo pass works on whole waves of envs).
constexpr int64_t kSmallRows = 16384;
int row_tiles_for(int64_t M, bool tick) { return (!tick && M <= kSmallRows) ? 1 : 2; }

// ---- LDS sizes ----
// Output-layer partial sums: [d_out <= 2][4 waves][TM rows] (red_floats per block).
__host__ __device__ constexpr int red_floats(int tm) { return 2 * kWaves * tm; }

// fp16 of gemm_cols_step's split stage for TM rows: [2 planes][TM][16], then the kWaves amax
// slots. A 32-row block keeps a region of the same size (two 32-row buffers, from the per-step
// form it once ran) ahead of its slots and never touches it: moving the slots would change every
// 32-row kernel's LDS immediates
__host__ __device__ constexpr size_t stage_halves(int tm) {
    return (size_t)(tm == 32 ? 2 : 1) * 2 * tm * 16;
}
// 32-row blocks also take the whole-layer stage past the slots (gemm_cols_whole): [hp / 16 k
// steps][2 planes][32][16] fp16, hp * 128 bytes
__host__ __device__ constexpr size_t stage_bytes(int tm, int hp) {
    return stage_halves(tm) * 2 + 4 * kWaves * (tm / 32) +
           (tm == 32 ? (size_t)hp * 128 : 0);
}

// rows [tm][hp+4] + input/dy staging [tm][4] + output-layer partial sums, then the split stage
__host__ __device__ constexpr size_t lds_floats(int hp, int tm) {
    return (size_t)tm * (hp + 4) + tm * 4 + red_floats(tm);
}
inline size_t lds_bytes(int hp, int tm) { return lds_floats(hp, tm) * 4 + stage_bytes(tm, hp); }
// bytes of the row kernels' LDS layout (lds_bytes) on the device side: the test rollout parks its
// two loop flags right behind it
__host__ __device__ constexpr size_t lds_bytes_c(int hp, int tm) {
    return lds_floats(hp, tm) * 4 + stage_bytes(tm, hp);
}
// host: the launch sizes of what the td3_*_rows_body.inc kernels carve up. critic_rows keeps,
// between the partial sums and the stage, the sampled rows [tm][8], q1' [tm] and the row
// backward's dL/dq rows [tm][4]; actor_rows the two dy row sets [tm][4] each; its BC forms, past
// the stage, the rows' actions [2][tm] and the waves' BC sums
constexpr size_t critic_rows_lds(int tm, int hp) {
    return (lds_floats(hp, tm) + tm * 8 + tm + tm * 4) * 4 + stage_bytes(tm, hp);
}
constexpr size_t actor_rows_lds(int tm, int hp) {
    return (lds_floats(hp, tm) + tm * 8) * 4 + stage_bytes(tm, hp);
}
constexpr size_t actor_rows_bc_lds(int tm, int hp) {
    return actor_rows_lds(tm, hp) + (2 * tm + kBlock / 64) * 4;
}
// the Q-filtered BC form: past those, the rows' Q1(s, a_demo) [tm], later their keep flags
constexpr size_t actor_rows_bcq_lds(int tm, int hp) {
    return actor_rows_bc_lds(tm, hp) + tm * 4;
}

// ---- forward, test rollout, row backward ----
// One member of a population (nav_act_tick_pop / nav_test_rollout_pop): its actor, its constants
// and its replay ring. The device-resident table [n_members] is written once per population
// (nav_pop_table_build); a workgroup's rows all belong to one member, so its entry is read
// through a block-uniform pointer.
struct PopMember {
    MlpDev net;
    nav_params p;
    float4* rows;      // the member's ring (null in a table built without rings: test rollouts)
    int64_t base_off;  // (-m * envs_per_member) mod capacity: (replay_base + base_off) % capacity
                       // + global env index is the member-local slot, so push_row's and the demo
                       // pass's (base + e) % cap hold as they are
};

struct FwdArgs {
    MlpDev net[2];
    int64_t M;
    const float* in;
    int ld_in, in_col;
    float* out[2];
    int ld_out, out_col;
    float* acts[2];
    uint32_t save_mask;  // bit L: hidden layer L's output rows are copied to acts + L*M*hp
    uint16_t* masks[2];
    // OUT_LOSS: train_critic's online twin forward with the TD error and the output layer's
    // gradient partials (robot.py:341-361)
    const float* batch;  // [M][8] replay rows (r at 4, done at 7)
    const float* qt[2];  // target twin values q1', q2' [M]
    float gamma, norm;   // discount, 2/B (mse_loss backward)
    float* dq[2];        // [M] dL/dq
    float* loss_part[2]; // [blocks] sum of (q - y)^2 over the block's rows
    float* eslab[2];     // [blocks][edge_count]: Wo / bo partials (nullable)
    int64_t ecount;
    // OUT_TARGET
    const float* eps;
    float policy_noise, noise_clip, max_action;
    uint32_t seed_lo, seed_hi, counter;
    // IN_BASELINE / OUT_ACT
    const double* state;
    const double* goal;
    const double* noise_scale;
    const double* noise_z;
    uint32_t step;
    int act_mode;
    double max_action_d;
    double* action_out;
    // OUT_TICK: the training tick of every row's env with the action just formed (one launch:
    // nav_act + nav_agent_step(_indexed); nav_act_tick)
    nav_params p;
    nav_env_soa env;
    const float2* field;
    float4* rows;
    int64_t cap, base;
    nav_step_out sout;
    DemoIdx demo;
    double* reward_out;
    // OUT_TICK_POP: the member table and the workgroups per member (net[0], rows and
    // max_action_d above are then unused and p carries the members' common seed only; cap is
    // the members' common capacity, base the common replay_base % cap)
    const PopMember* pop;
    int32_t pop_blocks;
};

// ---------------- greedy test episodes (robot-learning.py:78, 104-117) ----------------
struct TestArgs {
    MlpDev net;              // the actor (2 -> 2)
    int64_t n;
    const double2* goal;     // env->goal
    const double4* region;   // env->region (read only when start is null)
    const double2* start;    // nullable [n]
    const float2* field;
    double max_action, goal_threshold;
    uint32_t seed_lo, seed_hi, episode;
    int32_t max_steps;
    nav_test_out out;
    // k_test_rollout<.., POP>: the member table and the workgroups per member (net, max_action and
    // goal_threshold above are then unused)
    const PopMember* pop;
    int32_t pop_blocks;
};

// ---------------- row-local backward ----------------
struct BwdArgs {
    MlpDev net[2];           // 1 or 2 networks (blockIdx.y), same shapes, same input rows
    int64_t M;
    const float* dy[2];
    int ld_dy;               // dy row stride (0: one row broadcast to every row)
    const uint16_t* masks[2];
    const float* in;         // the forward's input rows (dW0 partials), with eslab
    int ld_in, in_col;
    const float* h_top[2];   // nullable: [M][hp] top activations -> Wo / bo partials here
    float* dz[2];            // [n_hidden][M][hp], layers with a save_mask bit written
    uint32_t save_mask;
    float* dx[2];
    float* eslab[2];         // nullable: [blocks][edge_count] W0 / bias (/ Wo / bo) partials
    int64_t ecount;
};

// ---- L2 warmers for small grids ----
// A 32-row workgroup streams every weight image it multiplies by (hp^2 + hp floats per layer)
// and, alone on its XCD at small batches, each k step's B fragments arrive from beyond its L2 at
// one CU's fetch rate (~75 GB/s: ~500 cycles per step of 6 MFMAs at hp = 224, flat in the
// prefetch depth; profiles/r06za). The row kernels therefore launch, when the compute grid leaves
// most CUs idle, extra workgroup rows (blockIdx.y >= y0) that only touch one 4-B word per 128-B
// line of the launch's images, in the order the compute workgroups consume them, so the lines
// are in each XCD's L2 before the compute workgroups ask. Blocks are dealt round-robin over the
// 8 XCDs (MI355X_MICROARCH: b and b + 8 share one; speed only, never correctness): the warmers
// with equal (index mod 8) split the image list between them (warm_l2, td3_rows.h).
constexpr int kWarmMax = 16;         // image ranges per launch
constexpr int kWarmPerXcd = 16;      // warmer workgroups per XCD
constexpr int64_t kWarmGrid = 128;   // compute workgroups up to which warmers are launched
struct WarmList {
    int y0;                          // grid rows of compute workgroups (warmers: rows >= y0)
    int n;                           // ranges (0: no warmers)
    const char* p[kWarmMax];
    uint32_t bytes[kWarmMax];
};

// host: append [p, p + bytes) to the list; false when full
inline bool warm_add(WarmList& w, const float* p, int64_t floats) {
    if (w.n >= kWarmMax) return false;
    w.p[w.n] = reinterpret_cast<const char*>(p);
    w.bytes[w.n++] = (uint32_t)(floats * 4);
    return true;
}
// host: a network's forward images (layers 1 .. nh-1), or its whole packed buffer (all images)
inline bool warm_net(WarmList& w, const MlpDev& net, bool fwd_only) {
    if (net.n_hidden < 2) return true;
    const int64_t im = split_image_floats(net.hp);
    if (!fwd_only) return warm_add(w, net.packed, (int64_t)(net.n_hidden - 1) * 2 * im);
    for (int L = 1; L < net.n_hidden; ++L)
        if (!warm_add(w, net.packed + (int64_t)(L - 1) * 2 * im, im)) return false;
    return true;
}
// host: grid rows of warmers for a compute grid of gx x gy (0: none)
inline unsigned warm_rows(const WarmList& w, unsigned gx, unsigned gy) {
    if (w.n == 0 || (int64_t)gx * gy > kWarmGrid) return 0;
    return (8u * kWarmPerXcd + gx - 1) / gx;
}

// ---------------- fused TD3 row programs ----------------
struct CriticRowsArgs {
    MlpDev actor_t, critic_t[2], critic[2];
    int64_t B;
    const float* rows;
    int64_t rsize;
    const int64_t* idx;
    uint32_t seed_lo, seed_hi, sample_ctr, noise_ctr;
    const float* eps;
    float policy_noise, noise_clip, max_action, gamma, norm;
    float* batch;
    float* dq[2];
    float* loss_part[2];
    float* eslab[2];
    int64_t ecount;
    float* acts[2];
    uint32_t save_mask;
    uint16_t* masks[2];
    int row_backward;     // also each online critic's row backward (robot.py:361 .backward())
    int split_twins;      // grid.y = 2: workgroup y runs online critic y only (small batches)
    float* dz[2];         // [nh][B][hp] dz rows of dz_save_mask layers (row_backward)
    uint32_t dz_save_mask;
    WarmList warm;        // set by the launcher
};
static_assert(sizeof(CriticRowsArgs) <= 4096, "kernel argument size");

// The population forms of critic_rows / actor_rows (nav_td3_critic_rows_pop / _actor_rows_pop):
// grid.z is the member, whose CriticRowsArgs / ActorRowsArgs the workgroup reads from the device
// table (nav_td3_pop_table_build) through a block-uniform pointer. What changes per launch and is
// common to all members travels by value, so the table is not rewritten while training: the
// replay fill, the Philox counter, and the twins' form (chosen from all members' workgroups).
struct RowsPop {
    const void* table;  // [n_members] CriticRowsArgs or ActorRowsArgs
    int64_t size;
    uint32_t counter;
    int32_t split_twins;
};

// The weighted form (nav_td3_critic_rows_w, prioritised replay): the plain arguments and, beside
// them, the rows' importance weights and the |TD error| outputs. Not in CriticRowsArgs: the
// population table stores that struct per member.
struct CriticPerExtra {
    const float* w;      // [B] importance weights
    float* td_abs[2];    // [B] |q_i - y| per online critic
};
struct CriticRowsWArgs {
    CriticRowsArgs r;
    CriticPerExtra per;
};
static_assert(sizeof(CriticRowsWArgs) <= 4096, "kernel argument size");

struct ActorRowsArgs {
    MlpDev actor, critic;
    int64_t B;
    const float* rows;
    int64_t rsize;
    const int64_t* idx;
    uint32_t seed_lo, seed_hi, sample_ctr;
    float dq;            // d(-mean Q)/dQ = -1/B
    float* batch;        // [B][8] sampled rows
    float* q;            // [B] Q1(s, pi(s)), nullable
    float* da;           // [B][2] dL/da
    float* acts;         // actor [nh][B][hp], save_mask layers (the top one feeds dWo)
    uint32_t save_mask;
    float* dz;           // actor [nh][B][hp], dz_save_mask layers
    uint32_t dz_save_mask;
    uint16_t* masks_a;
    uint16_t* masks_c;
    float* eslab;        // actor edge partials
    int64_t ecount;
    WarmList warm;       // set by the launcher
};

// The behaviour-cloning forms of actor_rows (nav_td3_actor_rows_bc): the plain arguments (dq =
// -q_weight/B) and, beside them, what the BC term on the batch's first B_demo rows needs. Not in
// ActorRowsArgs: the population table stores that struct per member.
enum { ACTOR_PLAIN = 0, ACTOR_TD3_BC = 1, ACTOR_BC_ONLY = 2, ACTOR_TD3_BCQ = 3 };
struct ActorBcExtra {
    int64_t B_demo;      // rows b < B_demo are demonstration rows
    float bc_coef;       // 2 * bc_weight / B_demo
    float* bc_part;      // [row blocks] block sums of (pi_j - a_j)^2 over demonstration rows
};
struct ActorRowsBcArgs {
    ActorRowsArgs r;     // r.critic: the actor's descriptor again when bc_only (never read)
    ActorBcExtra bc;
    int bc_only;         // no critic given: the BC term alone
};
// The Q-filtered BC form (nav_td3_actor_rows_bcq, MODE = ACTOR_TD3_BCQ): a demonstration row b <
// B_demo adds its BC term only where keep_b = Q1(s_b, a_b) > Q1(s_b, pi(s_b)) (online critic 1,
// strict; a NaN on either side compares false: dropped). The decision carries no gradient, and
// the term's normaliser stays B_demo, not the kept rows' count: bc_coef stays a launch constant
// and no count crosses the blocks before the backward pass. Not in ActorBcExtra: the
// population's BC table stores ActorRowsBcArgs per member.
struct ActorBcqExtra {
    float* q_demo;       // [B] Q1(s, a_demo), rows < B_demo written; nullable
    int32_t* keep_part;  // [row blocks] demonstration rows of the block the filter kept
};
struct ActorRowsBcqArgs {
    ActorRowsBcArgs b;   // bc_only 0: the filter needs the critic
    ActorBcqExtra qf;
};

// what a population launch passes to the per-NT objects (the table's row sections are
// [n_members] CriticRowsArgs, then [n_members] ActorRowsArgs; the BC table's is [n_members]
// ActorRowsBcArgs)
struct RowsPopLaunch {
    RowsPop k;
    int64_t B;
    int n_hidden, n_members;
};

}  // namespace
