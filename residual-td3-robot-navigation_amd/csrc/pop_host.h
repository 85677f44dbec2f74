// pop_host.h — what the population entry points of every object share on the host (no device
// code): the member limit, the "all members have member 0's shape" check and the writer of a
// host-built table into device memory.
#pragma once
#include "nav_device.h"

// `bytes` (a multiple of 4) of a host-built table to device memory `dev`, as by-value kernel
// arguments in 2 KB chunks: stream-ordered, and no host memory outlives the call
// (pop_state.hip). 0 or the negated HIP error.
int navi_table_write(const void* host, int64_t bytes, void* dev, hipStream_t st);

// nav_td3_mix_idx_pop's launch (learner_pop.hip) after mlp_abi.hip's checks: `mix` is the BC
// table's [n_members] MixMember section
int navi_mix_idx_pop_launch(const void* mix, int32_t n_members, int64_t B, int64_t size,
                            int64_t demo_base, uint32_t counter, int32_t actor_too,
                            hipStream_t st);

namespace nav {

constexpr int kMaxMembers = 256;

// One member's entry of the BC table's second section (nav_td3_pop_bc_table_build writes it in
// mlp_abi.hip, k_td3_mix_idx_pop reads it in learner_pop.hip): what nav_td3_mix_idx takes per
// member; the fill, the counter, B and the common capacity travel with the launch.
struct MixMember {
    int64_t B_demo, n_demo;
    uint32_t s0, s1;
    int64_t* out[2];  // idx_critic, idx_actor
};
static_assert(sizeof(MixMember) % 8 == 0, "the table's sections stay 8-byte aligned");

inline bool same_net_shape(const nav_mlp& a, const nav_mlp& b) {
    return a.d_in == b.d_in && a.d_out == b.d_out && a.hidden == b.hidden &&
           a.hidden_pad == b.hidden_pad && a.n_hidden == b.n_hidden;
}

// 1 <= n <= kMaxMembers learners, each of the six networks shaped as member 0's and one ring
// capacity
inline bool members_same_shape(const nav_td3_member* members, int32_t n) {
    if (!members || n < 1 || n > kMaxMembers) return false;
    const nav_td3_member& t0 = members[0];
    for (int m = 1; m < n; ++m) {
        const nav_td3_member& t = members[m];
        if (!same_net_shape(t.actor, t0.actor) ||
            !same_net_shape(t.target_actor, t0.target_actor) ||
            t.replay.capacity != t0.replay.capacity)
            return false;
        for (int i = 0; i < 2; ++i)
            if (!same_net_shape(t.critics[i], t0.critics[i]) ||
                !same_net_shape(t.target_critics[i], t0.target_critics[i]))
                return false;
    }
    return true;
}

}  // namespace nav
