// pop_host.h — what the population entry points of every object share on the host (no device
// code): the member limit, the "all members have member 0's shape" check and the writer of a
// host-built table into device memory.
#pragma once
#include "nav_device.h"

// `bytes` (a multiple of 4) of a host-built table to device memory `dev`, as by-value kernel
// arguments in 2 KB chunks: stream-ordered, and no host memory outlives the call
// (pop_state.hip). 0 or the negated HIP error.
int navi_table_write(const void* host, int64_t bytes, void* dev, hipStream_t st);

namespace nav {

constexpr int kMaxMembers = 256;

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
