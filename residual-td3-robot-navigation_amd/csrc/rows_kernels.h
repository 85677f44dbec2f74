// rows_kernels.h — the single-pass row kernels: k_mlp_fwd (a forward with its output modes: plain
// rows, target policy smoothing, the TD loss, the action, the action and the env's tick in one
// launch), k_test_rollout (a whole greedy test episode per workgroup) and k_mlp_bwd (the row
// backward). Their argument structs and LDS sizes are rows_args.h's, the passes they run
// rows_layers.h's; the fused TD3 row programs are td3_rows.h.
#pragma once
#include "rows_layers.h"


namespace {

template <int NT, int RT, int IN_MODE, int OUT_MODE>
__global__ __launch_bounds__(kBlock, 1) void k_mlp_fwd(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int hp = NT * 32, SS = hp + 4, TM = RT * 32;
    const int tid = threadIdx.x;
    // OUT_TICK_POP: the tick of OUT_TICK with the workgroup's member's actor, constants and ring
    constexpr bool POP = OUT_MODE == OUT_TICK_POP, TICK = OUT_MODE == OUT_TICK || POP;
    const PopMember* pm = nullptr;
    if constexpr (POP) pm = a.pop + blockIdx.x / (unsigned)a.pop_blocks;
    const MlpDev& net = POP ? pm->net : a.net[blockIdx.y];
    float* act_save = a.acts[blockIdx.y];
    uint16_t* masks = a.masks[blockIdx.y];
    const int64_t M = a.M;
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    const int64_t rt0 = (int64_t)blockIdx.x * RT;
    const int64_t n_rt = mask_rowtiles(M);
    float* act = smem;
    float* xin = smem + TM * SS;  // [TM][4]
    _Float16* stage = reinterpret_cast<_Float16*>(smem + lds_floats(hp, TM));
    const int d_in = net.d_in, d_out = net.d_out;
    // layer 0's per-lane weights and bias: issued first, in flight under the input rows' loads
    const L0Pre l0 = load_l0<NT>(net);
    if constexpr (OUT_MODE == OUT_TICK) NAV_CLOCK(2, 0);
    // the member's ring, its base and its action bound: block-uniform loads ahead of the pass
    float4* prows = nullptr;
    int64_t pbase = 0;
    double pmax = 0.0;
    if constexpr (POP) {
        prows = pm->rows;
        pbase = (a.base + pm->base_off) % a.cap;
        pmax = pm->p.max_action;
    }

    // ---- input rows -> xin
    if (tid < TM) {
        const int64_t r = row0 + tid;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < M) {
            if (IN_MODE == IN_F32) {
                const float* src = a.in + r * a.ld_in + a.in_col;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < d_in) x[k] = src[k];
            } else {
                // robot.py:556 baseline = state - goal, then torch.FloatTensor (f64 -> f32)
                const double2 s = reinterpret_cast<const double2*>(a.state)[r];
                const double2 g = reinterpret_cast<const double2*>(a.goal)[r];
                x[0] = (float)(s.x - g.x);
                x[1] = (float)(s.y - g.y);
            }
        }
        *reinterpret_cast<float4*>(xin + tid * 4) = make_float4(x[0], x[1], x[2], x[3]);
    }
    // OUT_TICK: the row's tick inputs that do not depend on its action (state, goal, meta, the
    // plan counters, the stuck ring, the field value), its noise scale and exploration noise are
    // loaded / drawn now, so their latency hides under the network pass
    TickIn tin{};
    double nsc = 0.0;
    double2 zz = make_double2(0.0, 0.0);
    if constexpr (TICK) {
        const int64_t r = row0 + tid;
        if (tid < TM && r < M) {
            tin = tick_load(a.env, a.field, r);
            if (a.act_mode == 0) {
                nsc = a.noise_scale[r];
                if (a.noise_z)
                    zz = make_double2(a.noise_z[r * 2], a.noise_z[r * 2 + 1]);
                else
                    zz = gauss_pair(philox(0u, (uint32_t)r, NAV_TAG_NOISE, a.step, a.p.seed_lo,
                                           a.p.seed_hi));
            }
        }
    }
    __syncthreads();

    float* red = xin + TM * 4;  // [2][PARTS][TM]
    f32x16 top[RT][2];
    fwd_net<NT, RT, kPfWide, IN_MODE == IN_BASELINE ? 2 : 0>(net, act, stage, xin, red, masks, n_rt, act_save, a.save_mask, row0, M, rt0, top,
                    TICK ? NAV_TICK_MK : -64, &l0);
    const int rloc = tid % TM;
    const int j = tid / TM;
    const int64_t r = row0 + rloc;
    if (OUT_MODE == OUT_LOSS) {
        // robot.py:341-345 TD target y = r + gamma * min(q1', q2') * (1 - done)
        float yt = 0.f;
        if (tid < TM && r < M) {
            const float rw = a.batch[r * NAV_ROW + 4], dn = a.batch[r * NAV_ROW + 7];
            const float mn = fminf(a.qt[0][r], a.qt[1][r]);
            yt = rw + (a.gamma * mn) * (1.0f - dn);
        }
        const int q = blockIdx.y;
        loss_epilogue<NT, RT>(net, top, red, row0, M, yt, a.norm, a.dq[q],
                              a.loss_part[q] + blockIdx.x,
                              a.eslab[q] ? a.eslab[q] + (int64_t)blockIdx.x * a.ecount : nullptr);
        return;
    }
    if constexpr (TICK) {
        // robot.py:556-567 as OUT_ACT, the action parked in LDS (the input rows are done with),
        // then the tick of env row0 + t by thread t < TM: nav_agent_step's device code
        // the row's thread forms both action components (the same expressions per component as
        // OUT_ACT) and runs its env's tick; no LDS round trip, no barrier in between
        DemoPend pend{false, false, 0.0, make_double2(0.0, 0.0)};
        TickStats st{0.f, 0.f, 0.f, 0.f, 0.f};
        NAV_TRACE_MARK(NAV_TICK_MK + 6);
        if (tid < TM && r < M) {
            double v[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const float y = out_y<RT>(net, red, tid, jj);
                const double sj = jj == 0 ? tin.s.x : tin.s.y, gj = jj == 0 ? tin.g.x : tin.g.y;
                double c = (sj - gj) + (double)y;
                if constexpr (POP) {
                    if (a.act_mode == 0) c = c + (nsc * pmax) * (jj == 0 ? zz.x : zz.y);
                    v[jj] = clipd(c, -pmax, pmax);
                } else {
                    if (a.act_mode == 0)
                        c = c + (nsc * a.max_action_d) * (jj == 0 ? zz.x : zz.y);
                    v[jj] = clipd(c, -a.max_action_d, a.max_action_d);
                }
                if (a.action_out) a.action_out[r * 2 + jj] = v[jj];
            }
            const double2 av = make_double2(v[0], v[1]);
            // (the plain tick's statements stand beside the member's, not merged with them
            // through selects: merged, its scalar loads came out of the compiler elsewhere)
            if constexpr (POP)
                st = a.demo.cand ? agent_tick_in<true>(pm->p, a.env, r, tin, av, prows, a.cap,
                                                       pbase, a.sout, true, pend)
                                 : agent_tick_in<false>(pm->p, a.env, r, tin, av, prows, a.cap,
                                                        pbase, a.sout, false, pend);
            else
                st = a.demo.cand ? agent_tick_in<true>(a.p, a.env, r, tin, av, a.rows, a.cap,
                                                       a.base, a.sout, true, pend)
                                 : agent_tick_in<false>(a.p, a.env, r, tin, av, a.rows, a.cap,
                                                        a.base, a.sout, false, pend);
        }
        NAV_TRACE_MARK(NAV_TICK_MK + 7);
        if (a.demo.cand) {  // block-uniform: the demo pass of the block's envs, all threads
            // the LDS rows are done with (the actions live in xin)
            auto* scratch = reinterpret_cast<DemoScratch<TM, kBlock>*>(act);
            if constexpr (POP) {
                const double rd = demo_pass<TM, kBlock>(pm->p, a.demo, *scratch, pend, r,
                                                        reinterpret_cast<float*>(prows), a.cap,
                                                        pbase, a.reward_out);
                if (pend.need) st.r = (float)rd;
            } else {
                const double rd = demo_pass<TM, kBlock>(a.p, a.demo, *scratch, pend, r,
                                                        reinterpret_cast<float*>(a.rows), a.cap,
                                                        a.base, a.reward_out);
                if (pend.need) st.r = (float)rd;  // the final reward of a flagged env
            }
        }
        NAV_TRACE_MARK(NAV_TICK_MK + 8);
        if (tid < TM && a.sout.block_stats && row0 + (tid & ~63) < M)
            wave_stats(st, a.sout.block_stats, r);
        NAV_TRACE_MARK(NAV_TICK_MK + 9);
        NAV_CLOCK(2, 1);
        return;
    }
    if (r >= M || j >= d_out) return;
    const float y = out_y<RT>(net, red, rloc, j);
    if (OUT_MODE == OUT_F32) {
        a.out[blockIdx.y][r * a.ld_out + a.out_col + j] = y;
    } else if (OUT_MODE == OUT_TARGET) {
        // robot.py:338-339 target policy smoothing
        float e;
        if (a.eps) {
            e = a.eps[r * 2 + j];
        } else {
            const double2 z = gauss_pair(philox((uint32_t)r, 0u, NAV_TAG_TNOISE, a.counter,
                                                a.seed_lo, a.seed_hi));
            e = (float)(j == 0 ? z.x : z.y);
        }
        float nz = e * a.policy_noise;
        nz = fminf(fmaxf(nz, -a.noise_clip), a.noise_clip);
        float v = y + nz;
        v = fminf(fmaxf(v, -a.max_action), a.max_action);
        a.out[blockIdx.y][r * a.ld_out + a.out_col + j] = v;
    } else {
        // robot.py:556-567 (training) / 586-593 (testing)
        const double s = a.state[r * 2 + j], g = a.goal[r * 2 + j];
        double c = (s - g) + (double)y;
        if (a.act_mode == 0) {
            double z;
            if (a.noise_z) {
                z = a.noise_z[r * 2 + j];
            } else {
                const double2 zz = gauss_pair(philox(0u, (uint32_t)r, NAV_TAG_NOISE, a.step,
                                                     a.seed_lo, a.seed_hi));
                z = j == 0 ? zz.x : zz.y;
            }
            c = c + (a.noise_scale[r] * a.max_action_d) * z;
        }
        a.action_out[r * 2 + j] = clipd(c, -a.max_action_d, a.max_action_d);
        if (a.out[0]) a.out[0][r * 2 + j] = y;
    }
}

// ---------------- greedy test episodes (robot-learning.py:78, 104-117) ----------------
// One workgroup = TM envs for a whole test episode: thread t < TM keeps env row0 + t's state,
// goal, best distance, step count and reached flag in registers and, per step, writes the
// baseline input row, takes its residual from the block's forward (fwd_net, as k_mlp_fwd), forms
// the testing-mode action (OUT_ACT's expressions, no noise) and moves (k_env_step's). A row that
// has reached its goal keeps its state: its input row then repeats, it still takes part in the
// GEMMs and barriers, and its results are dropped. The block leaves the loop when no row runs;
// the two LDS flags alternate by step parity, so a step costs one barrier on top of fwd_net's
// (step t's runners raise flag t & 1 while thread 0 clears the other, which was last read a
// step ago and is next raised a step ahead, both behind fwd_net's barriers).
// POP (nav_test_rollout_pop): the workgroup's member's actor, max_action and goal_threshold from
// the member table; the start draw stays keyed by the global env index and the common seed.
template <int NT, int RT, bool POP = false>
__global__ __launch_bounds__(kBlock, 1) void k_test_rollout(TestArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int hp = NT * 32, SS = hp + 4, TM = RT * 32;
    const int tid = threadIdx.x;
    const PopMember* pm = nullptr;
    if constexpr (POP) pm = a.pop + blockIdx.x / (unsigned)a.pop_blocks;
    const MlpDev& net = POP ? pm->net : a.net;
    double pmax = 0.0, pthr = 0.0;  // block-uniform loads, once, outside the step loop
    if constexpr (POP) {
        pmax = pm->p.max_action;
        pthr = pm->p.goal_threshold;
    }
    const int64_t n = a.n, row0 = (int64_t)blockIdx.x * TM, r = row0 + tid;
    float* act = smem;
    float* xin = smem + TM * SS;   // [TM][4]
    float* red = xin + TM * 4;     // [2][PARTS][TM]
    _Float16* stage = reinterpret_cast<_Float16*>(smem + lds_floats(hp, TM));
    int* flag = reinterpret_cast<int*>(reinterpret_cast<char*>(smem) + lds_bytes_c(hp, TM));
    // layer 0's per-lane weights and bias: once, outside the step loop
    const L0Pre l0 = load_l0<NT>(net);
    const bool mine = tid < TM && r < n;
    double2 s = make_double2(0.0, 0.0), g = s;
    if (mine) {
        g = a.goal[r];
        if (a.start) {
            s = a.start[r];
        } else {
            // Environment.reset's formula (environment.py:130-137) on the test stream
            const uint4 w = philox(0u, (uint32_t)r, NAV_TAG_TEST, a.episode, a.seed_lo, a.seed_hi);
            const double4 rg = a.region[r];
            const double reg[4] = {rg.x, rg.y, rg.z, rg.w};
            s = region_sample(reg, u01(w.x, w.y), u01(w.z, w.w));
        }
    }
    double best = __builtin_huge_val();
    int32_t steps = a.max_steps;
    uint8_t reached = 0;
    bool run = mine;
    double2* traj = reinterpret_cast<double2*>(a.out.traj);
    if (tid == 0) flag[0] = flag[1] = 0;
    __syncthreads();
    int t = 1;
    for (; t <= a.max_steps; ++t) {
        // robot.py:586-588 baseline = state - goal, then torch.FloatTensor (f64 -> f32)
        if (tid < TM)
            *reinterpret_cast<float4*>(xin + tid * 4) =
                mine ? make_float4((float)(s.x - g.x), (float)(s.y - g.y), 0.f, 0.f)
                     : make_float4(0.f, 0.f, 0.f, 0.f);
        if (run) flag[t & 1] = 1;
        if (tid == 0) flag[(t + 1) & 1] = 0;
        // the row's field value does not depend on its action: in flight under the network pass
        float2 fv = make_float2(0.f, 0.f);
        if (run) fv = field_at(a.field, s);
        __syncthreads();
        if (!__builtin_amdgcn_readfirstlane(flag[t & 1])) break;  // block-uniform
        f32x16 top[RT][2];
        fwd_net<NT, RT, kPfWide, 2>(net, act, stage, xin, red, nullptr, 0, nullptr, 0u, row0, n, 0,
                                    top, -64, &l0);
        if (run) {
            // robot.py:589-593, mode 1 (both components by the row's thread, as OUT_TICK)
            double v[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const float y = out_y<RT>(net, red, tid, jj);
                const double sj = jj == 0 ? s.x : s.y, gj = jj == 0 ? g.x : g.y;
                const double max_action = POP ? pmax : a.max_action;
                v[jj] = clipd((sj - gj) + (double)y, -max_action, max_action);
            }
            // environment.py:122-127
            const double2 nx = dynamics_f(fv, s, make_double2(v[0], v[1]));
            if (in_world(nx)) s = nx;
            // robot-learning.py:107, 113-114
            const double d = norm2(s.x - g.x, s.y - g.y);
            best = d < best ? d : best;
            if (d <= (POP ? pthr : a.goal_threshold)) {
                reached = 1;
                steps = t;
                run = false;
            }
        }
        if (traj && mine) traj[(int64_t)(t - 1) * n + r] = s;
    }
    if (!mine) return;
    // steps the block did not take: the final state repeats
    if (traj)
        for (int64_t k = t - 1; k < a.max_steps; ++k) traj[k * n + r] = s;
    a.out.reached[r] = reached;
    a.out.steps[r] = steps;
    a.out.best_distance[r] = best;
    reinterpret_cast<double2*>(a.out.final_state)[r] = s;
}

// ---------------- row-local backward ----------------
template <int NT, int RT, int BM>
__global__ __launch_bounds__(kBlock, 1) void k_mlp_bwd(BwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int hp = NT * 32, SS = hp + 4, TM = RT * 32;
    const int tid = threadIdx.x;
    const int y = blockIdx.y;
    const MlpDev& net = a.net[y];
    const int64_t M = a.M;
    const int64_t row0 = (int64_t)blockIdx.x * TM;
    const int64_t rt0 = (int64_t)blockIdx.x * RT;
    const int64_t n_rt = mask_rowtiles(M);
    float* act = smem;
    _Float16* stage = reinterpret_cast<_Float16*>(smem + lds_floats(hp, TM));
    float* dys = smem + TM * SS;  // [TM][4] dy rows
    float* xin = dys + TM * 4;    // [TM][4] forward input rows (dW0), inside the red scratch
    const int d_in = net.d_in, d_out = net.d_out;
    static_assert(hp <= kBlock, "one thread per hidden column");
    float* es = a.eslab[y] ? a.eslab[y] + (int64_t)blockIdx.x * a.ecount : nullptr;

    if (tid < TM) {
        const int64_t r = row0 + tid;
        float x[2] = {0.f, 0.f};
        float xi[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < M) {
            for (int j = 0; j < d_out; ++j) x[j] = a.dy[y][r * a.ld_dy + j];
            if (es)
                for (int k = 0; k < d_in; ++k) xi[k] = a.in[r * a.ld_in + a.in_col + k];
        }
        *reinterpret_cast<float4*>(dys + tid * 4) = make_float4(x[0], x[1], 0.f, 0.f);
        *reinterpret_cast<float4*>(xin + tid * 4) = make_float4(xi[0], xi[1], xi[2], xi[3]);
    }
    __syncthreads();
    bwd_net<NT, RT, 1, BM>(net, act, stage, dys, xin, a.masks[y], n_rt, es, a.h_top[y], a.dz[y],
                           a.save_mask, row0, M, rt0);

    // dx = dz_0 . W0 : thread = (row, input)
    if (a.dx[y]) {
        const int rloc = tid % TM;
        const int64_t r = row0 + rloc;
        for (int jj = tid / TM; jj < d_in; jj += kBlock / TM) {
            const float v = dx_unit<NT>(net, act, rloc, jj);
            if (r < M) a.dx[y][r * d_in + jj] = v;
        }
    }
}

}  // namespace
