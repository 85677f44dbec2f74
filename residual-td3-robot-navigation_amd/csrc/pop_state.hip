// pop_state.hip — population-based training on one device: the per-member scores of a population
// test rollout (nav_pop_test_summary) and the cloning of learners inside a population
// (nav_td3_pop_state_build, nav_td3_pop_exploit), and the writer of every host-built population
// table (navi_table_write, pop_host.h). A translation unit of its own: every other
// object of libnavenv.so compiles from the source and with the flags it had before.
#include <stdlib.h>

#include "pop_host.h"

namespace {

using namespace nav;

// ---------------- scores ----------------
// One workgroup per member: thread t folds envs t, t + 256, .. of the member in that order, then a
// fixed tree over the 256 partials in LDS. The order of every sum depends on envs_per_member
// alone, so two calls agree bit for bit and member m's score does not depend on n_members.
__global__ __launch_bounds__(kBlock) void k_pop_test_summary(
    const uint8_t* __restrict__ reached, const int32_t* __restrict__ steps,
    const double* __restrict__ best, int32_t envs_per_member, nav_pop_score* __restrict__ scores) {
    __shared__ double s_sum[kBlock], s_max[kBlock];
    __shared__ long long s_n[kBlock], s_steps[kBlock];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * envs_per_member;
    double sum = 0.0, mx = -HUGE_VAL;
    long long n = 0, st = 0;
    for (int e = t; e < envs_per_member; e += kBlock) {
        const double b = best[base + e];
        sum += b;
        mx = b > mx ? b : mx;
        if (reached[base + e]) {
            n += 1;
            st += steps[base + e];
        }
    }
    s_sum[t] = sum;
    s_max[t] = mx;
    s_n[t] = n;
    s_steps[t] = st;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (t < o) {
            s_sum[t] += s_sum[t + o];
            s_max[t] = s_max[t + o] > s_max[t] ? s_max[t + o] : s_max[t];
            s_n[t] += s_n[t + o];
            s_steps[t] += s_steps[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        nav_pop_score r;
        r.reached = s_n[0];
        r.steps_reached = s_steps[0];
        r.sum_best = s_sum[0];
        r.max_best = s_max[0];
        scores[blockIdx.x] = r;
    }
}

// ---------------- learner state ----------------
// A member's learner state as 19 segments, each a whole number of 16-byte units: the six
// networks' params, their packed images, the six Adam moments, the replay ring.
constexpr int kNets = 6;
constexpr int kSegs = 3 * kNets + 1;
constexpr int kRing = kSegs - 1;

struct StateMember {
    uint4* seg[kSegs];
    int64_t units[kSegs];  // 16-byte units of seg[i]; the ring's entry is its whole capacity
};
static_assert(sizeof(StateMember) % 8 == 0, "the table stays 8-byte aligned");

// the pairs of one launch, by value: word j = src | dst << 16
struct PairList {
    uint32_t w[kMaxMembers];
};

// Grid (chunk blocks, pairs). The pair and with it every segment pointer and size are
// block-uniform; a thread walks the concatenated range of all segments in 16-byte units with the
// grid's stride. A launch never reads what it writes (no dst among the src), so no order is needed.
// The table's pointers are device memory: named as such, so that the copies are global (not flat)
// dwordx4 loads and stores.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

__global__ void k_pop_exploit(const StateMember* __restrict__ tab, PairList pairs,
                              int64_t ring_units) {
    const uint32_t w = pairs.w[blockIdx.y];
    const StateMember& s = tab[w & 0xFFFFu];
    const StateMember& d = tab[w >> 16];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // in the concatenated range
    int64_t start = 0;
    for (int i = 0; i < kSegs; ++i) {
        const int64_t n = i == kRing ? ring_units : s.units[i];
        const int64_t end = start + n;
        const g_u32x4* from = (const g_u32x4*)s.seg[i];
        g_u32x4* to = (g_u32x4*)d.seg[i];
        for (; pos + 3 * stride < end; pos += 4 * stride) {
            const int64_t at = pos - start;
            const u32x4 a = from[at], b = from[at + stride], c = from[at + 2 * stride],
                        e = from[at + 3 * stride];
            to[at] = a;
            to[at + stride] = b;
            to[at + 2 * stride] = c;
            to[at + 3 * stride] = e;
        }
        for (; pos < end; pos += stride) to[pos - start] = from[pos - start];
        start = end;
    }
}

// 2 KB of kernel argument per write of a table (navi_table_write)
constexpr int kChunkWords = 512;
struct StateChunk {
    uint32_t w[kChunkWords];
};
__global__ void k_state_chunk_write(StateChunk c, uint32_t* dst, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = c.w[i];
}

bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

void member_nets(const nav_td3_member& t, const nav_mlp* (&nets)[kNets]) {
    nets[0] = &t.actor;
    nets[1] = &t.critics[0];
    nets[2] = &t.critics[1];
    nets[3] = &t.target_actor;
    nets[4] = &t.target_critics[0];
    nets[5] = &t.target_critics[1];
}

// The host check the state entry points share (before any HIP call); dst (nullable):
// [n_members] host entries
int state_check(const nav_td3_member* members, int32_t n_members, StateMember* dst) {
    if (!members_same_shape(members, n_members)) return NAV_EINVAL;
    const nav_mlp* nets0[kNets];
    member_nets(members[0], nets0);
    int64_t params16[kNets], packed16[kNets];
    for (int i = 0; i < kNets; ++i) {
        const nav_mlp& n = *nets0[i];
        if (n.hidden < 1 || n.hidden > n.hidden_pad) return NAV_EINVAL;
        const int64_t count = nav_mlp_param_count(n.d_in, n.d_out, n.hidden_pad, n.n_hidden);
        const int64_t packed = nav_mlp_packed_count(n.hidden_pad, n.n_hidden);
        if (count < 4 || packed < 0 || (count & 3) || (packed & 3)) return NAV_EINVAL;
        params16[i] = count / 4;
        packed16[i] = packed / 4;
    }
    const int64_t cap = members[0].replay.capacity;
    if (cap < 1 || cap > ((int64_t)1 << 40)) return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        const nav_td3_member& t = members[m];
        const nav_mlp* nets[kNets];
        member_nets(t, nets);
        float* const moments[kNets] = {t.m_actor,     t.m_critic[0], t.m_critic[1],
                                       t.v_actor,     t.v_critic[0], t.v_critic[1]};
        StateMember e{};
        for (int i = 0; i < kNets; ++i) {
            if (!aligned16(nets[i]->params) || !aligned16(moments[i])) return NAV_EINVAL;
            if (packed16[i] && !aligned16(nets[i]->packed)) return NAV_EINVAL;
            e.seg[i] = reinterpret_cast<uint4*>(nets[i]->params);
            e.units[i] = params16[i];
            e.seg[kNets + i] = packed16[i] ? reinterpret_cast<uint4*>(nets[i]->packed) : nullptr;
            e.units[kNets + i] = packed16[i];
            // a moment buffer has its network's size: m / v of the actor, critic 1, critic 2
            e.seg[2 * kNets + i] = reinterpret_cast<uint4*>(moments[i]);
            e.units[2 * kNets + i] = params16[i % 3];
        }
        if (!aligned16(t.replay.rows)) return NAV_EINVAL;
        e.seg[kRing] = reinterpret_cast<uint4*>(t.replay.rows);
        e.units[kRing] = cap * 2;  // 32-byte rows
        if (dst) dst[m] = e;
    }
    return 0;
}

}  // namespace

int navi_table_write(const void* host, int64_t bytes, void* dev, hipStream_t st) {
    const uint32_t* words = static_cast<const uint32_t*>(host);
    const int64_t total = bytes / 4;
    for (int64_t at = 0; at < total; at += kChunkWords) {
        StateChunk c;
        const int n = (int)(total - at < kChunkWords ? total - at : kChunkWords);
        for (int i = 0; i < n; ++i) c.w[i] = words[at + i];
        hipLaunchKernelGGL(k_state_chunk_write, dim3(1), dim3(kBlock), 0, st, c,
                           static_cast<uint32_t*>(dev) + at, n);
        NAV_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" {

int nav_pop_test_summary(const nav_test_out* out, int32_t n_members, int32_t envs_per_member,
                         nav_pop_score* scores, void* stream) {
    if (!out || !scores || n_members < 1 || n_members > kMaxMembers || envs_per_member < 64 ||
        envs_per_member % 64 != 0 || !out->reached || !out->steps || !out->best_distance)
        return NAV_EINVAL;
    hipLaunchKernelGGL(k_pop_test_summary, dim3((unsigned)n_members), dim3(kBlock), 0, S(stream),
                       out->reached, out->steps, out->best_distance, envs_per_member, scores);
    NAV_CHECK_LAUNCH();
    return 0;
}

int64_t nav_td3_pop_state_bytes(int32_t n_members) {
    if (n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    return (int64_t)n_members * (int64_t)sizeof(StateMember);
}

int nav_td3_pop_state_build(const nav_td3_member* members, int32_t n_members, void* state_table,
                            void* stream) {
    if (!state_table || n_members < 1 || n_members > kMaxMembers) return NAV_EINVAL;
    StateMember* host = static_cast<StateMember*>(calloc((size_t)n_members, sizeof(StateMember)));
    if (!host) return NAV_EINVAL;
    int rc = state_check(members, n_members, host);
    if (!rc)
        rc = navi_table_write(host, (int64_t)n_members * (int64_t)sizeof(StateMember), state_table,
                              S(stream));
    free(host);
    return rc;
}

int nav_td3_pop_exploit(const nav_td3_member* members, int32_t n_members,
                        const void* state_table, const int32_t* src, const int32_t* dst,
                        int32_t n_pairs, int64_t replay_rows, void* stream) {
    if (!state_table || !src || !dst || n_members < 1 || n_members > kMaxMembers ||
        n_pairs < 1 || n_pairs > n_members - 1)
        return NAV_EINVAL;
    // 0: in neither list, 1: a source, 2: a destination
    uint8_t role[kMaxMembers] = {0};
    PairList pairs{};
    for (int j = 0; j < n_pairs; ++j) {
        const int32_t s = src[j], d = dst[j];
        if (s < 0 || s >= n_members || d < 0 || d >= n_members || s == d) return NAV_EINVAL;
        if (role[d] != 0 || role[s] == 2) return NAV_EINVAL;
        role[s] = 1;
        role[d] = 2;
        pairs.w[j] = (uint32_t)s | ((uint32_t)d << 16);
    }
    StateMember e0[1];
    int rc = state_check(members, 1, e0);  // the common sizes
    if (!rc) rc = state_check(members, n_members, nullptr);
    if (rc) return rc;
    if (replay_rows < 0 || replay_rows > members[0].replay.capacity) return NAV_EINVAL;
    int64_t total = replay_rows * 2;
    for (int i = 0; i < kRing; ++i) total += e0[0].units[i];
    // four units per thread in flight; at most ~8 workgroups per CU over all pairs
    int64_t gx = (total + 4 * kBlock - 1) / (4 * kBlock);
    const int64_t cap = (8 * kCUs) / n_pairs;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_pop_exploit, dim3((unsigned)gx, (unsigned)n_pairs), dim3(kBlock), 0,
                       S(stream), static_cast<const StateMember*>(state_table), pairs,
                       replay_rows * 2);
    NAV_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
