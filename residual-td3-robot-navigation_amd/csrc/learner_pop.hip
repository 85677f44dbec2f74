// learner_pop.hip — the population learner's cross-row kernels and their C ABI: the kernels of
// learner_kernels.hip with one more grid dimension, the member (blockIdx.y). A workgroup reads its
// member's argument struct from the device table through a block-uniform pointer and runs the
// same body (wgrad.h, reduce_adam.h) on it. An object of its own (learner_pop.o), so the plain
// kernels' object holds what it held before. Also the population's demonstration mix
// (k_td3_mix_idx_pop), launched for mlp_abi.hip's nav_td3_mix_idx_pop.
#include "learner_host.h"

namespace {

struct LearnMember {
    WgradArgs wg[2];   // group 0: the twin critics, group 1: the actor
    RedArgs red[3];    // the critics' step, the actor's, the actor's with the three soft updates
    PackArgs pack[3];  // the images each of those rewrites (<= 4 networks)
    double lr[2];      // critic_lr, actor_lr: step_size = (float)(lr / bc1) on the device
};
static_assert(sizeof(LearnMember) % 4 == 0, "copied as 32-bit words");

template <bool GEN>
__global__ __launch_bounds__(WG_THREADS) void k_wgrad_pop(const LearnMember* __restrict__ tab,
                                                          int group) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const WgradArgs& a = tab[blockIdx.y].wg[group];
    wgrad_tile<GEN>(a, wgrad_job(a, blockIdx.x, gridDim.x), smem);
}
template <int NI, int D, int KH>
__global__ __launch_bounds__(WG_THREADS) void k_wgrad_fact_pop(const LearnMember* __restrict__ tab,
                                                               int group) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ uint4 ftab[256];
    const WgradArgs& a = tab[blockIdx.y].wg[group];
    wgrad_tile_fact<NI, D, KH>(a, wgrad_job(a, blockIdx.x, gridDim.x), smem, ftab);
}

__global__ __launch_bounds__(kBlock) void k_grad_reduce_adam_pop(
    const LearnMember* __restrict__ tab, int which, AdamStep st, double bc1) {
    const LearnMember& m = tab[blockIdx.y];
    // lr / (1 - b1^t) in f64, then to f32: the host's two roundings (_Adam.advance, c_float)
    st.step_size = (float)(m.lr[which ? 1 : 0] / bc1);
    grad_reduce_body<true, true>(m.red[which], st);
}

__global__ __launch_bounds__(kBlock) void k_pack_img_pop(const LearnMember* __restrict__ tab,
                                                         int set) {
    const PackArgs& a = tab[blockIdx.y].pack[set];
#include "pack_img_body.inc"
}

// k_td3_mix_idx (learner_kernels.hip) with the member on grid.y: member m's seed, B_demo, n_demo
// and index arrays from its MixMember, the same Philox draws and the same two formulas
struct MixPopArgs {
    const MixMember* tab;
    int64_t size, B, demo_base;
    uint32_t ctr0;
    int32_t actor_too;
};
__global__ __launch_bounds__(kBlock) void k_td3_mix_idx_pop(MixPopArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.B) return;
    const MixMember& m = a.tab[blockIdx.y];
    const bool demo = b < m.B_demo;
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (y == 1 && !a.actor_too) continue;
        const uint4 w = philox((uint32_t)b, 0u, demo ? NAV_TAG_DEMO : NAV_TAG_SAMPLE,
                               a.ctr0 + (uint32_t)y, m.s0, m.s1);
        m.out[y][b] = demo ? a.demo_base + (int64_t)(((uint64_t)w.x * (uint64_t)m.n_demo) >> 32)
                           : (int64_t)(((uint64_t)w.x * (uint64_t)a.size) >> 32);
    }
}

// One member's entry (every check of the single-member entry points on the way); blocks[w]: grid.x
// of reduce launch w
int learn_member_fill(const nav_td3_member& t, int64_t B, int32_t sc, int32_t sa, LearnMember& e,
                      int (&blocks)[3]) {
    if (B < 1 || sc < 1 || sa < 1 || !t.batch || !t.batch_actor || !t.da) return NAV_EINVAL;
    const int64_t nblk = nav_mlp_row_blocks(B);
    const nav_mlp crit[2] = {t.critics[0], t.critics[1]};
    const nav_mlp tcrit[2] = {t.target_critics[0], t.target_critics[1]};
    if (t.actor.n_hidden != t.critics[0].n_hidden || t.actor.d_in != 2 || t.actor.d_out != 2 ||
        crit[0].d_in != 4 || crit[0].d_out != 1 || crit[1].d_in != 4 || crit[1].d_out != 1)
        return NAV_EINVAL;
    if (t.actor.n_hidden > 1) {
        int rc = wgrad_args(crit, 2, B, t.batch, 8, 0, t.acts, t.dz, t.dq, 1, t.masks,
                            t.hidden_slabs, sc, e.wg[0]);
        if (rc) return rc;
        const float* acts_a[1] = {t.acts_actor};
        const float* dz_a[1] = {t.dz_actor};
        const float* dy_a[1] = {t.da};
        const uint16_t* mk_a[1] = {t.masks_actor};
        float* hs_a[1] = {t.hidden_slabs[0]};
        rc = wgrad_args(&t.actor, 1, B, t.batch_actor, 8, 0, acts_a, dz_a, dy_a, 2, mk_a, hs_a,
                        sa, e.wg[1]);
        if (rc) return rc;
    }
    const float zero[2] = {0.f, 0.f};
    PackSet ps[3];
    int rc = red_args(crit, 2, t.hidden_slabs, sc, t.edge_slabs, nblk, t.grad_critic, t.m_critic,
                      t.v_critic, 0.f, 0.f, 0.f, zero, zero, nullptr, nullptr, nullptr, 0, 0.f,
                      e.red[0], &blocks[0], &ps[0]);
    if (rc) return rc;
    const float* hs_a[1] = {t.hidden_slabs[0]};
    const float* es_a[1] = {t.edge_slabs_actor};
    float* g_a[1] = {t.grad_actor};
    float* m_a[1] = {t.m_actor};
    float* v_a[1] = {t.v_actor};
    rc = red_args(&t.actor, 1, hs_a, sa, es_a, nblk, g_a, m_a, v_a, 0.f, 0.f, 0.f, zero, zero,
                  nullptr, nullptr, nullptr, 0, 0.f, e.red[1], &blocks[1], &ps[1]);
    if (rc) return rc;
    rc = red_args(&t.actor, 1, hs_a, sa, es_a, nblk, g_a, m_a, v_a, 0.f, 0.f, 0.f, zero, zero,
                  &t.target_actor, tcrit, crit, 2, t.tau, e.red[2], &blocks[2], &ps[2]);
    if (rc) return rc;
    for (int w = 0; w < 3; ++w) {
        ps[w].shape();
        e.pack[w] = ps[w].a;
    }
    e.lr[0] = t.critic_lr;
    e.lr[1] = t.actor_lr;
    return 0;
}

// the check every entry point shares; e0 / blocks: member 0's entry (the launch shape)
int learn_pop_check(const nav_td3_member* members, int32_t n_members, int64_t B, int32_t sc,
                    int32_t sa, LearnMember* dst, LearnMember& e0, int (&blocks)[3]) {
    if (!members_same_shape(members, n_members) || B < 1) return NAV_EINVAL;
    for (int m = 0; m < n_members; ++m) {
        const nav_td3_member& t = members[m];
        LearnMember e{};
        int bl[3] = {0, 0, 0};
        const int rc = learn_member_fill(t, B, sc, sa, e, bl);
        if (rc) return rc;
        if (m == 0) {
            e0 = e;
            for (int w = 0; w < 3; ++w) blocks[w] = bl[w];
        }
        if (dst) dst[m] = e;
    }
    return 0;
}

// the table's second section: past the members' row-kernel arguments
const LearnMember* learn_section(const void* table, int32_t n_members) {
    return reinterpret_cast<const LearnMember*>(static_cast<const char*>(table) +
                                                (int64_t)n_members * navi_rows_pop_entry_bytes());
}

}  // namespace

int64_t navi_learner_pop_entry_bytes() { return (int64_t)sizeof(LearnMember); }

int navi_learner_pop_fill(const nav_td3_member* members, int32_t n_members, int64_t B,
                          int32_t splits_critic, int32_t splits_actor, void* dst) {
    LearnMember e0;
    int blocks[3];
    return learn_pop_check(members, n_members, B, splits_critic, splits_actor,
                           static_cast<LearnMember*>(dst), e0, blocks);
}

int navi_mix_idx_pop_launch(const void* mix, int32_t n_members, int64_t B, int64_t size,
                            int64_t demo_base, uint32_t counter, int32_t actor_too,
                            hipStream_t st) {
    MixPopArgs a{static_cast<const MixMember*>(mix), size, B, demo_base, 2u * counter,
                 actor_too ? 1 : 0};
    hipLaunchKernelGGL(k_td3_mix_idx_pop, dim3((unsigned)blocks_for(B), (unsigned)n_members),
                       dim3(kBlock), 0, st, a);
    NAV_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int32_t nav_mlp_wgrad_splits_pop(int32_t n_members, int32_t n_nets, int32_t d_out,
                                 int32_t hidden_pad, int32_t n_hidden, int64_t M) {
    if (n_members < 1 || n_members > kMaxMembers || n_nets < 1 || n_nets > 2 || d_out < 1 ||
        d_out > 2 || hidden_pad < 32 || hidden_pad > 256 || (hidden_pad & 31) || n_hidden < 1 ||
        M < 0)
        return NAV_EINVAL;
    return wgrad_splits((int64_t)n_members * n_nets, d_out, hidden_pad, n_hidden, M);
}

int nav_mlp_wgrad_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                      const void* table, int32_t group, int32_t splits, void* stream) {
    LearnMember e0;
    int blocks[3];
    if (!table || group < 0 || group > 1 || splits < 1) return NAV_EINVAL;
    const int rc = learn_pop_check(members, n_members, B, group == 0 ? splits : 1,
                                   group == 1 ? splits : 1, nullptr, e0, blocks);
    if (rc) return rc;
    if (members[0].actor.n_hidden < 2) return 0;
    const WgradArgs& a = e0.wg[group];
    const int n_nets = group == 0 ? 2 : 1;
    const int64_t per_member = (int64_t)n_nets * a.n_hid * splits;
    void (*const k[5])(const LearnMember*, int) = {
        k_wgrad_fact_pop<8, 1, 1>, k_wgrad_fact_pop<4, 1, 2>, k_wgrad_fact_pop<2, 1, 2>,
        k_wgrad_pop<true>, k_wgrad_pop<false>};
    return wgrad_launch(a, k, dim3((unsigned)per_member, (unsigned)n_members), S(stream),
                        learn_section(table, n_members), (int)group);
}

int nav_grad_reduce_adam_pop(const nav_td3_member* members, int32_t n_members, int64_t B,
                             const void* table, int32_t group, float beta1, float beta2,
                             float eps, double bc1, float bc2_sqrt, int32_t soft_update,
                             void* stream) {
    LearnMember e0;
    int blocks[3];
    if (!table || group < 0 || group > 1 || (soft_update && group != 1) || !(bc1 > 0.0) ||
        !(bc2_sqrt > 0.f))
        return NAV_EINVAL;
    const int rc = learn_pop_check(members, n_members, B, 1, 1, nullptr, e0, blocks);
    if (rc) return rc;
    const int which = group == 0 ? 0 : soft_update ? 2 : 1;
    AdamStep st{};
    st.bc2s = bc2_sqrt;
    set_adam(st, beta1, beta2, eps);
    const LearnMember* tab = learn_section(table, n_members);
    hipLaunchKernelGGL(k_grad_reduce_adam_pop, dim3((unsigned)blocks[which], (unsigned)n_members),
                       dim3(kBlock), 0, S(stream), tab, which, st, bc1);
    NAV_CHECK_LAUNCH();
    const PackArgs& pk = e0.pack[which];
    if (pk.n == 0) return 0;  // n_hidden == 1: no packed image
    hipLaunchKernelGGL(k_pack_img_pop, dim3((unsigned)(pk.n * pk.per_net), (unsigned)n_members),
                       dim3(kBlock), 0, S(stream), tab, which);
    NAV_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
