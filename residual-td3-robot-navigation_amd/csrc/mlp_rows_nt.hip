// mlp_rows_nt.hip — the launchers of the row kernels (mlp_rows.h) of one hidden width, hp = 32 *
// NAV_MLP_PART, and one role (NAV_MLP_ROLE, mlp_rows_role.h): 8 x 7 independent objects, so make
// -j compiles the heavy template instantiations in parallel. Each exports one dispatcher,
// nav_mlp_rows_<role>_<NT>(), that mlp_abi.hip calls; the role decides which kernels the object
// instantiates.
#include "mlp_rows_role.h"

namespace {

// every launch: the kernel's dynamic LDS limit, then the kernel
template <typename A>
void launch_k(void (*k)(A), dim3 grid, size_t lds, hipStream_t st, const A& a) {
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(k, grid, dim3(kBlock), lds, st, a);
}

unsigned row_blocks(int64_t M, int tm) { return (unsigned)((M + tm - 1) / tm); }

// The L2 warmers of a gx x gy compute grid: `n` networks' images in the order the compute
// workgroups consume them (fwd_only: the forward images alone), as grid rows from gy up. Returns
// the rows to add to the grid; 0 (and an empty list) when the grid needs none or the list is full.
struct WarmNet {
    const MlpDev& net;
    bool fwd_only;
};
unsigned set_warmers(WarmList& w, const WarmNet* nets, int n, unsigned gx, unsigned gy) {
    w = WarmList{};
    bool ok = true;
    for (int i = 0; ok && i < n; ++i) ok = warm_net(w, nets[i].net, nets[i].fwd_only);
    if (!ok) w.n = 0;
    w.y0 = (int)gy;
    const unsigned wy = warm_rows(w, gx, gy);
    if (wy == 0) w.n = 0;
    return wy;
}

template <int NT, int RT, int IN_MODE, int OUT_MODE>
void launch_fwd(const FwdArgs& a, int n_nets, hipStream_t st) {
    launch_k(k_mlp_fwd<NT, RT, IN_MODE, OUT_MODE>, dim3(row_blocks(a.M, RT * 32), (unsigned)n_nets),
             lds_bytes(NT * 32, RT * 32), st, a);
}

template <int NT, int RT>
void launch_bwd(const BwdArgs& a, int n_nets, hipStream_t st) {
    // d_out = 1 networks' top backward image is the Wt image: their top product is gemm_bits
    const int nh = a.net[0].n_hidden;
    auto k = a.net[0].d_out != 1 || nh < 2 ? k_mlp_bwd<NT, RT, 0>
             : nh == 2                      ? k_mlp_bwd<NT, RT, 2>
                                            : k_mlp_bwd<NT, RT, 1>;
    launch_k(k, dim3(row_blocks(a.M, RT * 32), (unsigned)n_nets), lds_bytes(NT * 32, RT * 32), st,
             a);
}

// critic_rows and actor_rows: the critics' row-backward form is 1 also for 2 hidden layers (its
// gemm_cols loop then runs no layer): the form-2 instantiation came out at 286 registers (one
// workgroup per CU), form 1 at 236
template <int NT, int RT>
void launch_critic_rows(const CriticRowsArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.critic[0].n_hidden == 1 ? k_td3_critic_rows<NT, RT, 0> : k_td3_critic_rows<NT, RT, 1>;
    const unsigned gx = row_blocks(a.B, TM), gy = a.split_twins ? 2u : 1u;
    CriticRowsArgs w = a;
    // (the targets: forward only)
    const WarmNet nets[] = {{a.actor_t, true}, {a.critic_t[0], true}, {a.critic_t[1], true},
                            {a.critic[0], false}, {a.critic[1], false}};
    const unsigned wy = set_warmers(w.warm, nets, 5, gx, gy);
    launch_k(k, dim3(gx, gy + wy), critic_rows_lds(TM, NT * 32), st, w);
}

template <int NT, int RT>
void launch_actor_rows(const ActorRowsArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.critic.n_hidden == 1 ? k_td3_actor_rows<NT, RT, 0> : k_td3_actor_rows<NT, RT, 1>;
    const unsigned gx = row_blocks(a.B, TM);
    ActorRowsArgs w = a;
    const WarmNet nets[] = {{a.actor, false}, {a.critic, false}};
    const unsigned wy = set_warmers(w.warm, nets, 2, gx, 1u);
    launch_k(k, dim3(gx, 1u + wy), actor_rows_lds(TM, NT * 32), st, w);
}

// the weighted form (prioritised replay): the plain form's grid, warmers and LDS
template <int NT, int RT>
void launch_critic_rows_w(const CriticRowsWArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.r.critic[0].n_hidden == 1 ? k_td3_critic_rows_w<NT, RT, 0>
                                         : k_td3_critic_rows_w<NT, RT, 1>;
    const unsigned gx = row_blocks(a.r.B, TM), gy = a.r.split_twins ? 2u : 1u;
    CriticRowsWArgs w = a;
    const WarmNet nets[] = {{a.r.actor_t, true}, {a.r.critic_t[0], true}, {a.r.critic_t[1], true},
                            {a.r.critic[0], false}, {a.r.critic[1], false}};
    const unsigned wy = set_warmers(w.r.warm, nets, 5, gx, gy);
    launch_k(k, dim3(gx, gy + wy), critic_rows_lds(TM, NT * 32), st, w);
}

// the BC forms; bc_only warms the actor's images alone
template <int NT, int RT>
void launch_actor_rows_bc(const ActorRowsBcArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.bc_only                ? k_td3_actor_rows_bc<NT, RT, 1, ACTOR_BC_ONLY>
             : a.r.critic.n_hidden == 1 ? k_td3_actor_rows_bc<NT, RT, 0, ACTOR_TD3_BC>
                                        : k_td3_actor_rows_bc<NT, RT, 1, ACTOR_TD3_BC>;
    const unsigned gx = row_blocks(a.r.B, TM);
    ActorRowsBcArgs w = a;
    const WarmNet nets[] = {{a.r.actor, false}, {a.r.critic, false}};
    const unsigned wy = set_warmers(w.r.warm, nets, a.bc_only ? 1 : 2, gx, 1u);
    launch_k(k, dim3(gx, 1u + wy), actor_rows_bc_lds(TM, NT * 32), st, w);
}

// the Q-filtered BC form: the BC form's grid and warmers, its LDS and the rows' Q1(s, a_demo)
template <int NT, int RT>
void launch_actor_rows_bcq(const ActorRowsBcqArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.b.r.critic.n_hidden == 1 ? k_td3_actor_rows_bcq<NT, RT, 0>
                                        : k_td3_actor_rows_bcq<NT, RT, 1>;
    const unsigned gx = row_blocks(a.b.r.B, TM);
    ActorRowsBcqArgs w = a;
    const WarmNet nets[] = {{a.b.r.actor, false}, {a.b.r.critic, false}};
    const unsigned wy = set_warmers(w.b.r.warm, nets, 2, gx, 1u);
    launch_k(k, dim3(gx, 1u + wy), actor_rows_bcq_lds(TM, NT * 32), st, w);
}

// the population forms: grid.z = the member, no L2 warmer rows
template <int NT, int RT>
void launch_critic_rows_pop(const RowsPopLaunch& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.n_hidden == 1 ? k_td3_critic_rows_pop<NT, RT, 0> : k_td3_critic_rows_pop<NT, RT, 1>;
    launch_k(k, dim3(row_blocks(a.B, TM), a.k.split_twins ? 2u : 1u, (unsigned)a.n_members),
             critic_rows_lds(TM, NT * 32), st, a.k);
}

template <int NT, int RT>
void launch_actor_rows_pop(const RowsPopLaunch& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.n_hidden == 1 ? k_td3_actor_rows_pop<NT, RT, 0> : k_td3_actor_rows_pop<NT, RT, 1>;
    launch_k(k, dim3(row_blocks(a.B, TM), 1u, (unsigned)a.n_members), actor_rows_lds(TM, NT * 32),
             st, a.k);
}

// the population's BC form: the BC kernel's LDS, the population forms' grid
template <int NT, int RT>
void launch_actor_rows_bc_pop(const RowsPopLaunch& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    auto k = a.n_hidden == 1 ? k_td3_actor_rows_bc_pop<NT, RT, 0> : k_td3_actor_rows_bc_pop<NT, RT, 1>;
    launch_k(k, dim3(row_blocks(a.B, TM), 1u, (unsigned)a.n_members),
             actor_rows_bc_lds(TM, NT * 32), st, a.k);
}

template <int NT, int RT, bool POP>
void launch_test(const TestArgs& a, hipStream_t st) {
    constexpr int TM = RT * 32;
    launch_k(k_test_rollout<NT, RT, POP>, dim3(row_blocks(a.n, TM)),
             lds_bytes_c(NT * 32, TM) + 2 * sizeof(int),  // + the two loop flags
             st, a);
}

// ROLE is a template parameter so that the other roles' branches are discarded, not instantiated
template <int NT, int RT, int ROLE>
int rows_rt(int fam, int in_mode, int out_mode, const void* args, int n_nets, hipStream_t st) {
    if (rows_role(fam, out_mode) != ROLE) return NAV_EINVAL;
    if constexpr (ROLE == ROLE_BCQ) {
        launch_actor_rows_bcq<NT, RT>(*static_cast<const ActorRowsBcqArgs*>(args), st);
    } else if constexpr (ROLE == ROLE_PER) {
        launch_critic_rows_w<NT, RT>(*static_cast<const CriticRowsWArgs*>(args), st);
    } else if constexpr (ROLE == ROLE_BC) {
        launch_actor_rows_bc<NT, RT>(*static_cast<const ActorRowsBcArgs*>(args), st);
    } else if constexpr (ROLE == ROLE_BCPOP) {
        launch_actor_rows_bc_pop<NT, RT>(*static_cast<const RowsPopLaunch*>(args), st);
    } else if constexpr (ROLE == ROLE_LPOP) {
        const RowsPopLaunch& a = *static_cast<const RowsPopLaunch*>(args);
        if (fam == FAM_CRITIC_POP)
            launch_critic_rows_pop<NT, RT>(a, st);
        else
            launch_actor_rows_pop<NT, RT>(a, st);
    } else if constexpr (ROLE == ROLE_POP) {
        if (fam == FAM_TEST_POP) {
            launch_test<NT, RT, true>(*static_cast<const TestArgs*>(args), st);
        } else if constexpr (RT >= 2) {  // the population tick
            if (in_mode != IN_BASELINE) return NAV_EINVAL;
            launch_fwd<NT, RT, IN_BASELINE, OUT_TICK_POP>(*static_cast<const FwdArgs*>(args),
                                                          n_nets, st);
        } else {
            return NAV_EINVAL;
        }
    } else {
        switch (fam) {
            case FAM_FWD: {
                const FwdArgs& a = *static_cast<const FwdArgs*>(args);
                if (in_mode == IN_BASELINE && out_mode == OUT_ACT)
                    launch_fwd<NT, RT, IN_BASELINE, OUT_ACT>(a, n_nets, st);
                else if (in_mode == IN_BASELINE && out_mode == OUT_TICK) {
                    if constexpr (RT >= 2)
                        launch_fwd<NT, RT, IN_BASELINE, OUT_TICK>(a, n_nets, st);
                    else
                        return NAV_EINVAL;
                } else if (in_mode == IN_F32 && out_mode == OUT_F32)
                    launch_fwd<NT, RT, IN_F32, OUT_F32>(a, n_nets, st);
                else if (in_mode == IN_F32 && out_mode == OUT_TARGET)
                    launch_fwd<NT, RT, IN_F32, OUT_TARGET>(a, n_nets, st);
                else if (in_mode == IN_F32 && out_mode == OUT_LOSS)
                    launch_fwd<NT, RT, IN_F32, OUT_LOSS>(a, n_nets, st);
                else
                    return NAV_EINVAL;
                break;
            }
            case FAM_BWD: launch_bwd<NT, RT>(*static_cast<const BwdArgs*>(args), n_nets, st); break;
            case FAM_CRITIC:
                launch_critic_rows<NT, RT>(*static_cast<const CriticRowsArgs*>(args), st);
                break;
            case FAM_ACTOR:
                launch_actor_rows<NT, RT>(*static_cast<const ActorRowsArgs*>(args), st);
                break;
            case FAM_TEST:
                launch_test<NT, RT, false>(*static_cast<const TestArgs*>(args), st);
                break;
            default: return NAV_EINVAL;
        }
    }
    return 0;
}

}  // namespace

int NAV_ROWS_FN(NAV_MLP_ROLE, NAV_MLP_PART)(int fam, int rt, int in_mode, int out_mode,
                                            const void* args, int n_nets, hipStream_t st) {
    constexpr int NT = NAV_MLP_PART, ROLE = NAV_MLP_ROLE;
    return rt == 1 ? rows_rt<NT, 1, ROLE>(fam, in_mode, out_mode, args, n_nets, st)
                   : rows_rt<NT, 2, ROLE>(fam, in_mode, out_mode, args, n_nets, st);
}

// (a trace variant builds one part with NAV_PHASE_TRACE: tools/build_variant.sh)
#if defined(NAV_PHASE_TRACE) && NAV_MLP_ROLE == 0
extern "C" int nav_phase_trace_read(unsigned long long* host, int n) {
    const size_t bytes = sizeof(g_phase_trace);
    if (!host || (size_t)n * sizeof(unsigned long long) < bytes) return NAV_EINVAL;
    const hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_phase_trace), bytes);
    return e == hipSuccess ? 0 : -(int)e;
}
#endif

#if defined(NAV_CLOCK_STAMP) && NAV_MLP_PART == 8 && NAV_MLP_ROLE == 0
extern "C" int nav_clock_stamp_read(unsigned long long* host, int n) {
    const size_t bytes = sizeof(g_clock_stamp);
    if (!host || (size_t)n * sizeof(unsigned long long) < bytes) return NAV_EINVAL;
    const hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_clock_stamp), bytes);
    return e == hipSuccess ? 0 : -(int)e;
}
#endif
