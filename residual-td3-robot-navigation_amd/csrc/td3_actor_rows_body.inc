// k_td3_actor_rows' statements (td3_rows.h includes this once per form, as
// td3_critic_rows_body.inc). MODE (constexpr, ACTOR_PLAIN in the plain and population kernels)
// selects the behaviour-cloning forms of k_td3_actor_rows_bc, whose extras arrive in `bx`:
// ACTOR_TD3_BC adds the BC term's gradient on rows < bx.B_demo to dL/da, ACTOR_BC_ONLY also runs
// no critic pass. The plain forms' statements are what they were. POP with ACTOR_TD3_BC is
// k_td3_actor_rows_bc_pop: `a` and `bx` from the member's entry of the BC table.
// ACTOR_TD3_BCQ (k_td3_actor_rows_bcq, extras in `qx`) is ACTOR_TD3_BC with the Q-filter: a
// workgroup with demonstration rows (row0 < bx.B_demo: block-uniform, the rows are the batch's
// prefix) first runs the critic forward on (s, a_demo), and a row's BC term counts only where that
// value exceeds Q1(s, pi(s)). The term's normaliser stays B_demo (bc_coef a launch constant).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (!POP) {
        if (a.warm.n && (int)blockIdx.y >= a.warm.y0) {  // an L2 warmer row (small grids)
            warm_l2(a.warm);
            return;
        }
    }
    constexpr int hp = NT * 32, SS = hp + 4, TM = RT * 32;
    const int tid = threadIdx.x;
    const int64_t B = a.B, row0 = (int64_t)blockIdx.x * TM, rt0 = (int64_t)blockIdx.x * RT;
    const int64_t n_rt = mask_rowtiles(B);
    float* act = smem;
    float* xin = act + TM * SS;      // [TM][4] (s, pi(s))
    float* red = xin + TM * 4;       // [2][PARTS][TM]
    float* dys = red + red_floats(TM);  // [TM][4] critic dy
    float* dys2 = dys + TM * 4;      // [TM][4] actor dy = dL/da
    _Float16* stage = reinterpret_cast<_Float16*>(dys2 + TM * 4);  // gemm_cols' split stage
    // BC forms: the sampled rows' actions [2][TM] and the waves' BC sums, past the stage
    [[maybe_unused]] float* bca =
        reinterpret_cast<float*>(reinterpret_cast<char*>(stage) + stage_bytes(TM, hp));
    // ACTOR_TD3_BCQ: past those, the rows' Q1(s, a_demo) [TM], then (same slots, written by the
    // thread that read them) 1.f where the filter keeps the row's BC term, else 0.f
    [[maybe_unused]] float* qd = bca + 2 * TM + kBlock / 64;
    const L0Pre l0_a = load_l0<NT>(a.actor);  // in flight under the sampling
    NAV_CLOCK(1, 0);
    if (tid < TM) {
        const int64_t b = row0 + tid;
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (b < B) {
            if constexpr (POP)
                sample_row(a.rows, pv.size, a.idx, a.seed_lo, a.seed_hi, 2u * pv.counter + 1u, b,
                           lo, hi);
            else
                sample_row(a.rows, a.rsize, a.idx, a.seed_lo, a.seed_hi, a.sample_ctr, b, lo, hi);
            float4* dst = reinterpret_cast<float4*>(a.batch) + 2 * b;
            dst[0] = lo;
            dst[1] = hi;
        }
        if constexpr (MODE != ACTOR_PLAIN) {
            bca[tid] = lo.z;
            bca[TM + tid] = lo.w;
        }
        if constexpr (MODE == ACTOR_TD3_BCQ)  // (s, a_demo); the actor's forward reads s alone
            *reinterpret_cast<float4*>(xin + tid * 4) = lo;
        else
        *reinterpret_cast<float4*>(xin + tid * 4) = make_float4(lo.x, lo.y, 0.f, 0.f);  // s
        *reinterpret_cast<float4*>(dys + tid * 4) =
            make_float4(b < B ? a.dq : 0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if constexpr (MODE == ACTOR_TD3_BCQ) {
        // Q1(s, a_demo) of the block's rows, as critic_rows runs its target passes: no masks, no
        // saved rows, no top-layer state kept (a.masks_c is the later (s, pi(s)) pass's). The
        // actor's forward overwrites the rows and (after its barriers) the partial sums.
        if (row0 < bx.B_demo) {
            f32x16 topq[RT][2];
            fwd_net<NT, RT, 1, 4>(a.critic, act, stage, xin, red, nullptr, n_rt, nullptr, 0u, row0,
                                  B, rt0, topq);
            if (tid < TM) {
                const float v = out_y<RT>(a.critic, red, tid, 0);
                qd[tid] = v;
                if (qx.q_demo && row0 + tid < bx.B_demo) qx.q_demo[row0 + tid] = v;
            }
        }
    }
    // the actor's top hidden layer stays in registers until dL/da is known (its dWo partials)
    f32x16 topa[RT][2];
    fwd_net<NT, RT, 1, 2>(a.actor, act, stage, xin, red, a.masks_a, n_rt, a.acts, a.save_mask, row0, B, rt0,
                    topa, -64, &l0_a);
    // (ACTOR_BC_ONLY: a.critic is the actor's descriptor again and these loads are dead)
    const L0Pre l0_c = load_l0<NT>(a.critic);  // in flight under the action epilogue
    if (tid < 2 * TM) {
        const int rloc = tid % TM, j = tid / TM;
        xin[rloc * 4 + 2 + j] = row0 + rloc < B ? out_y<RT>(a.actor, red, rloc, j) : 0.f;
    }
    __syncthreads();
    if constexpr (MODE != ACTOR_BC_ONLY) {
    // the critic's top-layer ReLU bits and Wo columns go from its forward to its row backward in
    // registers (as in critic_rows)
    f32x16 top[RT][2];
    uint32_t top_bits[RT * 2];
    WoCols wo;
    fwd_net<NT, RT, 1, 4>(a.critic, act, stage, xin, red, a.masks_c, n_rt, nullptr, 0u, row0, B, rt0, top,
                    -64, &l0_c, top_bits, &wo);
    // One hidden layer (CBM == 0): fwd_net's top layer is layer 0 and it leaves top_bits unset;
    // the row backward below read them uninitialised (the one-hidden-layer learner did not repeat
    // its own results). The bits are those of `top`, layer 0's post-ReLU registers.
    if constexpr (CBM == 0) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint32_t bits = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) bits |= pos_bit(top[rt][j][i]) << i;
                top_bits[rt * 2 + j] = bits;
            }
    }
    if constexpr (MODE == ACTOR_TD3_BCQ) {
        // the filter's decision, from the value that goes to a.q: strict, NaN compares false
        if (tid < TM) {
            const float qp = out_y<RT>(a.critic, red, tid, 0);
            if (a.q && row0 + tid < B) a.q[row0 + tid] = qp;
            const bool keep = row0 + tid < bx.B_demo && qd[tid] > qp;
            qd[tid] = keep ? 1.f : 0.f;  // (read below after bwd_net's barriers)
        }
    } else {
    if (tid < TM && a.q && row0 + tid < B) a.q[row0 + tid] = out_y<RT>(a.critic, red, tid, 0);
    }
    bwd_net<NT, RT, 1, CBM>(a.critic, act, stage, dys, xin, a.masks_c, n_rt, nullptr, nullptr,
                                    nullptr, 0u, row0, B, rt0, -64, top_bits, &wo);
    }
    if constexpr (MODE == ACTOR_PLAIN) {
    if (tid < 2 * TM) {
        const int rloc = tid % TM, j = tid / TM;
        const int64_t r = row0 + rloc;
        const float v = r < B ? dx_unit<NT>(a.critic, act, rloc, 2 + j) : 0.f;
        dys2[rloc * 4 + j] = v;
        if (r < B) a.da[r * 2 + j] = v;
    }
    } else {
        // dL/da = the critic's part (none in ACTOR_BC_ONLY) + on demonstration rows
        // bc_coef * (pi_j - a_j); the block's sum of (pi_j - a_j)^2: the waves' sums here, added
        // in wave order after the barrier (loss_epilogue's order)
        float e2 = 0.f;
        if (tid < 2 * TM) {
            const int rloc = tid % TM, j = tid / TM;
            const int64_t r = row0 + rloc;
            float v = 0.f;
            if constexpr (MODE == ACTOR_TD3_BC || MODE == ACTOR_TD3_BCQ)
                v = r < B ? dx_unit<NT>(a.critic, act, rloc, 2 + j) : 0.f;
            bool term = r < bx.B_demo;
            if constexpr (MODE == ACTOR_TD3_BCQ) term = qd[rloc] != 0.f;  // 0 on rows >= B_demo
            if (term) {
                const float d = xin[rloc * 4 + 2 + j] - bca[j * TM + rloc];
                v += bx.bc_coef * d;
                e2 = d * d;
            }
            dys2[rloc * 4 + j] = v;
            if (r < B) a.da[r * 2 + j] = v;
        }
        const float w = wave_sum(e2);
        if ((tid & 63) == 0) bca[2 * TM + (tid >> 6)] = w;
        if constexpr (MODE == ACTOR_TD3_BCQ) {
            // the block's kept rows, counted once each (j == 0's threads: all in wave 0)
            static_assert(TM <= 64, "the rows' threads are one wave");
            const float kept = wave_sum(tid < TM ? qd[tid] : 0.f);
            if (tid == 0) qx.keep_part[blockIdx.x] = (int32_t)kept;
        }
    }
    if (tid < TM) {
        dys2[tid * 4 + 2] = 0.f;
        dys2[tid * 4 + 3] = 0.f;
    }
    __syncthreads();
    if constexpr (MODE != ACTOR_PLAIN) {
        if (tid == 0) {
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) sum += bca[2 * TM + k];
            bx.bc_part[blockIdx.x] = sum;
        }
    }
    // the actor's output layer gradient partials: dWo from its top-layer registers, dbo = column
    // sums of dL/da (bwd_net's order)
    float* es = a.eslab + (int64_t)blockIdx.x * a.ecount;
    wo_grad_regs<NT, RT>(a.actor, topa, dys2, 4, es);
    if (tid < 4) {
        float sb = 0.f;
        if (tid < a.actor.d_out)
            for (int rr = 0; rr < TM; ++rr) sb += dys2[rr * 4 + tid];
        es[e_bo(a.actor) + tid] = sb;
    }
    bwd_net<NT, RT>(a.actor, act, stage, dys2, xin, a.masks_a, n_rt, es, nullptr, a.dz, a.dz_save_mask,
                    row0, B, rt0, -64, nullptr, nullptr, false);
    NAV_CLOCK(1, 1);
