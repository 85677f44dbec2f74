// td3_rows.h — the fused TD3 row programs (the learner, robot.py:209-398): critic_rows and
// actor_rows with their population, weighted (prioritised replay), behaviour-cloning and
// Q-filtered forms, each kernel a few constants around one of the two bodies
// td3_critic_rows_body.inc / td3_actor_rows_body.inc, and the L2 warmer their spare workgroup
// rows run. Their argument structs, LDS sizes and the warmer list are rows_args.h's, the network
// passes rows_layers.h's.
#pragma once
#include "rows_layers.h"


namespace {

// ---------------- fused TD3 row programs ----------------
// Everything in train_critic / train_actor that is local to a batch row runs as one launch per
// row block, the rows staying in LDS between the network passes (the launches that remain are
// the cross-row reductions: weight gradients and their reduce + Adam).

// ReplayBuffer.sample (robot.py:98-115) of row b: injected index or Philox with replacement
NAV_DEV void sample_row(const float* rows, int64_t size, const int64_t* idx, uint32_t s0,
                        uint32_t s1, uint32_t ctr, int64_t b, float4& lo, float4& hi) {
    int64_t k;
    if (idx) {
        k = idx[b];
    } else {
        const uint4 w = philox((uint32_t)b, 0u, NAV_TAG_SAMPLE, ctr, s0, s1);
        k = (int64_t)(((uint64_t)w.x * (uint64_t)size) >> 32);
    }
    const float4* src = reinterpret_cast<const float4*>(rows) + 2 * k;
    lo = src[0];
    hi = src[1];
}

// the L2 warmer of a workgroup in the grid rows past the compute ones (WarmList, rows_args.h)
NAV_DEV void warm_l2(const WarmList& w) {
    const uint32_t j = blockIdx.x + gridDim.x * (blockIdx.y - (uint32_t)w.y0);
    const uint32_t nw = gridDim.x * (gridDim.y - (uint32_t)w.y0);
    const uint32_t cnt = (nw - (j & 7u) + 7u) >> 3, rank = j >> 3;  // warmers of this XCD
    uint32_t x = 0;
    for (int i = 0; i < w.n; ++i) {
        const uint32_t lines = (w.bytes[i] + 127u) >> 7;
        const uint32_t per = (lines + cnt - 1u) / cnt;
        const uint32_t l1 = min(lines, (rank + 1u) * per);
        const char* p = w.p[i];
#pragma unroll 4
        for (uint32_t l = rank * per + threadIdx.x; l < l1; l += kBlock)
            x ^= *reinterpret_cast<const uint32_t*>(p + ((size_t)l << 7));
    }
    asm volatile("" ::"v"(x));  // keeps the loads
}

// train_critic (robot.py:329-361) for one block of TM batch rows: sample, target policy
// smoothing through the target actor, twin target critics, TD target, then the twin online
// critics with mse_loss's gradient, the loss and the output layers' gradient partials, and
// (row_backward) each online critic's row backward with its W0 / bias partials right after its
// forward, while its rows and ReLU bits are fresh.
// CBM: the critics' row-backward form (bwd_net's BM: 0 for one hidden layer, else 1), chosen by
// the launcher from n_hidden
// The kernel's statements are td3_critic_rows_body.inc, once per form: the plain kernel's stay
// token for token what they were (its machine code is pinned, tools/isa_diff.py), the population
// form (POP) reads `a` from the member's table entry and the launch's values from `pv` (the
// entry's rsize, counters, split_twins and warm list are then unused).
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows(CriticRowsArgs a) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr bool WEIGHTED = false;
    constexpr CriticPerExtra px{};
#include "td3_critic_rows_body.inc"
}
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr bool WEIGHTED = false;
    constexpr CriticPerExtra px{};
    const CriticRowsArgs& a = static_cast<const CriticRowsArgs*>(pv.table)[blockIdx.z];
#include "td3_critic_rows_body.inc"
}
// the weighted form (WEIGHTED: loss_epilogue scales dq and the loss term by px.w and writes
// px.td_abs; everything downstream reads the weighted dq)
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows_w(CriticRowsWArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr bool WEIGHTED = true;
    const CriticRowsArgs& a = x.r;
    const CriticPerExtra& px = x.per;
#include "td3_critic_rows_body.inc"
}

// train_actor (robot.py:382-390) for one block of TM batch rows: sample, actor forward,
// critic-1 forward on (s, pi(s)), backward of -mean(Q) through critic 1 to its action input
// (critic grads discarded, as zero_grad does), and the actor's row backward with its edge
// partials.
// (td3_actor_rows_body.inc once per form, as k_td3_critic_rows)
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows(ActorRowsArgs a) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr int MODE = ACTOR_PLAIN;
    constexpr ActorBcExtra bx{};
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr int MODE = ACTOR_PLAIN;
    constexpr ActorBcExtra bx{};
    constexpr ActorBcqExtra qx{};
    const ActorRowsArgs& a = static_cast<const ActorRowsArgs*>(pv.table)[blockIdx.z];
#include "td3_actor_rows_body.inc"
}
// the BC forms (MODE = ACTOR_TD3_BC / ACTOR_BC_ONLY; the latter runs no critic pass, so its CBM
// is unused and the launcher takes 1)
template <int NT, int RT, int CBM, int MODE>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bc(ActorRowsBcArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    const ActorRowsArgs& a = x.r;
    const ActorBcExtra& bx = x.bc;
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}
// the Q-filtered BC form: in the workgroups that hold demonstration rows (row0 < B_demo, the
// batch's prefix) one more forward of the critic, on (s, a_demo), ahead of the actor's
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bcq(ActorRowsBcqArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr int MODE = ACTOR_TD3_BCQ;
    const ActorRowsArgs& a = x.b.r;
    const ActorBcExtra& bx = x.b.bc;
    const ActorBcqExtra& qx = x.qf;
#include "td3_actor_rows_body.inc"
}
// the population's BC form (nav_td3_actor_rows_bc_pop): grid.z is the member, whose
// ActorRowsBcArgs the workgroup reads from the BC table (nav_td3_pop_bc_table_build) through a
// block-uniform pointer; size and counter from `pv` as in k_td3_actor_rows_pop
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bc_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr int MODE = ACTOR_TD3_BC;
    const ActorRowsBcArgs& x = static_cast<const ActorRowsBcArgs*>(pv.table)[blockIdx.z];
    const ActorRowsArgs& a = x.r;
    const ActorBcExtra& bx = x.bc;
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}

}  // namespace
