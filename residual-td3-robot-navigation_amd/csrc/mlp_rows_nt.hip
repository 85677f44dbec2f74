// mlp_rows_nt.hip — the launchers of the row kernels (rows_kernels.h, td3_rows.h; their launch
// contract is rows_args.h) of one hidden width, hp = 32 *
// NAV_MLP_PART, and one role (NAV_MLP_ROLE, mlp_rows_role.h): 8 x 7 independent objects, so make
// -j compiles the heavy template instantiations in parallel. Each exports one dispatcher,
// nav_mlp_rows_<role>_<NT>(), that mlp_abi.hip calls; the role decides which kernels the object
// instantiates.
#include "mlp_rows.h"
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

// The warmed single-learner row programs (critic_rows, actor_rows and their forms) launch in one
// place: the instantiation by the critic's depth (k_one: one hidden layer), B rows' blocks x gy
// compute workgroups with the L2 warmer rows of `nets` on top, `lds` bytes of LDS. `w` is the
// launcher's own copy of the arguments and `warm` the WarmList embedded in it.
template <typename A>
void launch_warmed(void (*k_one)(A), void (*k_more)(A), int n_hidden, A& w, WarmList& warm,
                   int64_t B, int tm, unsigned gy, const WarmNet* nets, int n, size_t lds,
                   hipStream_t st) {
    const unsigned gx = row_blocks(B, tm);
    const unsigned wy = set_warmers(warm, nets, n, gx, gy);
    launch_k(n_hidden == 1 ? k_one : k_more, dim3(gx, gy + wy), lds, st, w);
}

// critic_rows and its weighted form (`r`: the plain arguments inside `w`). The critics'
// row-backward form is 1 also for 2 hidden layers (its gemm_cols loop then runs no layer): the
// form-2 instantiation came out at 286 registers (one workgroup per CU), form 1 at 236
template <int NT, int RT, typename A>
void launch_critic(void (*k_one)(A), void (*k_more)(A), A& w, CriticRowsArgs& r, hipStream_t st) {
    // (the targets: forward only)
    const WarmNet nets[] = {{r.actor_t, true}, {r.critic_t[0], true}, {r.critic_t[1], true},
                            {r.critic[0], false}, {r.critic[1], false}};
    launch_warmed(k_one, k_more, r.critic[0].n_hidden, w, r.warm, r.B, RT * 32,
                  r.split_twins ? 2u : 1u, nets, 5, critic_rows_lds(RT * 32, NT * 32), st);
}

template <int NT, int RT>
void launch_critic_rows(CriticRowsArgs w, hipStream_t st) {
    launch_critic<NT, RT>(k_td3_critic_rows<NT, RT, 0>, k_td3_critic_rows<NT, RT, 1>, w, w, st);
}

// the weighted form (prioritised replay): the plain form's grid, warmers and LDS
template <int NT, int RT>
void launch_critic_rows_w(CriticRowsWArgs w, hipStream_t st) {
    launch_critic<NT, RT>(k_td3_critic_rows_w<NT, RT, 0>, k_td3_critic_rows_w<NT, RT, 1>, w, w.r,
                          st);
}

// actor_rows and its BC forms (`r`: the plain arguments inside `w`): the actor's images warmed
// and, with n_warm 2, the critic's
template <int RT, typename A>
void launch_actor(void (*k_one)(A), void (*k_more)(A), A& w, ActorRowsArgs& r, int n_warm,
                  size_t lds, hipStream_t st) {
    const WarmNet nets[] = {{r.actor, false}, {r.critic, false}};
    launch_warmed(k_one, k_more, r.critic.n_hidden, w, r.warm, r.B, RT * 32, 1u, nets, n_warm, lds,
                  st);
}

template <int NT, int RT>
void launch_actor_rows(ActorRowsArgs w, hipStream_t st) {
    launch_actor<RT>(k_td3_actor_rows<NT, RT, 0>, k_td3_actor_rows<NT, RT, 1>, w, w, 2,
                     actor_rows_lds(RT * 32, NT * 32), st);
}

// the BC forms; bc_only runs no critic pass: CBM 1 at every depth, the actor's images alone warmed
template <int NT, int RT>
void launch_actor_rows_bc(ActorRowsBcArgs w, hipStream_t st) {
    constexpr size_t lds = actor_rows_bc_lds(RT * 32, NT * 32);
    if (w.bc_only)
        launch_actor<RT>(k_td3_actor_rows_bc<NT, RT, 1, ACTOR_BC_ONLY>,
                         k_td3_actor_rows_bc<NT, RT, 1, ACTOR_BC_ONLY>, w, w.r, 1, lds, st);
    else
        launch_actor<RT>(k_td3_actor_rows_bc<NT, RT, 0, ACTOR_TD3_BC>,
                         k_td3_actor_rows_bc<NT, RT, 1, ACTOR_TD3_BC>, w, w.r, 2, lds, st);
}

// the Q-filtered BC form: the BC form's grid and warmers, its LDS and the rows' Q1(s, a_demo)
template <int NT, int RT>
void launch_actor_rows_bcq(ActorRowsBcqArgs w, hipStream_t st) {
    launch_actor<RT>(k_td3_actor_rows_bcq<NT, RT, 0>, k_td3_actor_rows_bcq<NT, RT, 1>, w, w.b.r, 2,
                     actor_rows_bcq_lds(RT * 32, NT * 32), st);
}

// the population forms (the three launches are in rows_rt): grid.z = the member, no L2 warmer rows
template <int RT>
void launch_pop(void (*k_one)(RowsPop), void (*k_more)(RowsPop), const RowsPopLaunch& a,
                unsigned gy, size_t lds, hipStream_t st) {
    launch_k(a.n_hidden == 1 ? k_one : k_more,
             dim3(row_blocks(a.B, RT * 32), gy, (unsigned)a.n_members), lds, st, a.k);
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
    } else if constexpr (ROLE == ROLE_BCPOP) {  // the BC kernel's LDS, the population's grid
        launch_pop<RT>(k_td3_actor_rows_bc_pop<NT, RT, 0>, k_td3_actor_rows_bc_pop<NT, RT, 1>,
                       *static_cast<const RowsPopLaunch*>(args), 1u,
                       actor_rows_bc_lds(RT * 32, NT * 32), st);
    } else if constexpr (ROLE == ROLE_LPOP) {
        const RowsPopLaunch& a = *static_cast<const RowsPopLaunch*>(args);
        if (fam == FAM_CRITIC_POP)
            launch_pop<RT>(k_td3_critic_rows_pop<NT, RT, 0>, k_td3_critic_rows_pop<NT, RT, 1>, a,
                           a.k.split_twins ? 2u : 1u, critic_rows_lds(RT * 32, NT * 32), st);
        else
            launch_pop<RT>(k_td3_actor_rows_pop<NT, RT, 0>, k_td3_actor_rows_pop<NT, RT, 1>, a,
                           1u, actor_rows_lds(RT * 32, NT * 32), st);
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
