// k_td3_critic_rows' statements (td3_rows.h includes this once per form: `a` the arguments,
// POP and `pv` the population form's flag and launch values, WEIGHTED and `px` the weighted
// form's flag and extras: k_td3_critic_rows_w)
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
    float* xin = act + TM * SS;    // [TM][4] network input rows
    float* red = xin + TM * 4;     // [2][PARTS][TM] output partial sums
    float* brow = red + red_floats(TM);  // [TM][8] the sampled replay rows
    float* qv = brow + TM * 8;     // [TM] q1'
    float* dys = qv + TM;          // [TM][4] dL/dq rows of the row backward
    _Float16* stage = reinterpret_cast<_Float16*>(dys + TM * 4);  // gemm_cols' split stage
    NAV_MARK(0);
    NAV_CLOCK(0, 0);
    const L0Pre l0_at = load_l0<NT>(a.actor_t);  // in flight under the sampling
    // the sampled replay row of thread tid < TM: its gather is issued first, so it is in flight
    // while the smoothing noise below is formed
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (tid < TM && row0 + tid < B) {
        if constexpr (POP)
            sample_row(a.rows, pv.size, a.idx, a.seed_lo, a.seed_hi, 2u * pv.counter, row0 + tid,
                       lo, hi);
        else
            sample_row(a.rows, a.rsize, a.idx, a.seed_lo, a.seed_hi, a.sample_ctr, row0 + tid, lo, hi);
    }
    // target policy smoothing noise of (row, output) (tid - TM) % TM, (tid - TM) / TM: clamp(
    // policy_noise * eps, +-noise_clip) — threads past the sampling ones, so its f64 Box-Muller
    // runs on other waves (other SIMDs) than the sampling's Philox draw and gather
    static_assert(3 * TM <= kBlock, "sampling threads, then the noise's");
    float tnz = 0.f;
    const int tn = tid - TM;
    if (tn >= 0 && tn < 2 * TM && row0 + tn % TM < B) {
        const int64_t r = row0 + tn % TM;
        const int j = tn / TM;
        float e;
        if (a.eps) {
            e = a.eps[r * 2 + j];
        } else {
            uint32_t nctr;
            if constexpr (POP) nctr = pv.counter;
            else nctr = a.noise_ctr;
            const double2 z = gauss_pair(philox((uint32_t)r, 0u, NAV_TAG_TNOISE, nctr,
                                                a.seed_lo, a.seed_hi));
            e = (float)(j == 0 ? z.x : z.y);
        }
        tnz = fminf(fmaxf(e * a.policy_noise, -a.noise_clip), a.noise_clip);
    }
    if (tid < TM) {
        const int64_t b = row0 + tid;
        if (b < B && blockIdx.y == 0) {  // split twins: one writer per batch row
            float4* dst = reinterpret_cast<float4*>(a.batch) + 2 * b;
            dst[0] = lo;
            dst[1] = hi;
        }
        *reinterpret_cast<float4*>(brow + tid * 8) = lo;
        *reinterpret_cast<float4*>(brow + tid * 8 + 4) = hi;
        *reinterpret_cast<float4*>(xin + tid * 4) = make_float4(hi.y, hi.z, 0.f, 0.f);  // s'
    }
    __syncthreads();
    NAV_MARK(1);
    // target actor; a' = clamp(pi'(s') + clamp(policy_noise * eps, +-noise_clip), +-max_action).
    // Each pass's layer-0 constants are loaded one pass ahead (L0Pre).
    f32x16 top[RT][2];
    const L0Pre l0_ct1 = load_l0<NT>(a.critic_t[0]);
    fwd_net<NT, RT, kPfWide, 2>(a.actor_t, act, stage, xin, red, nullptr, n_rt, nullptr, 0u, row0, B, rt0, top, 2,
                    &l0_at);
    if (tn >= 0 && tn < 2 * TM) {  // the noise's threads
        const int rloc = tn % TM, j = tn / TM;
        const int64_t r = row0 + rloc;
        float v = 0.f;
        if (r < B) {
            const float y = out_y<RT>(a.actor_t, red, rloc, j);
            v = y + tnz;
            v = fminf(fmaxf(v, -a.max_action), a.max_action);
        }
        xin[rloc * 4 + 2 + j] = v;
    }
    __syncthreads();
    NAV_MARK(8);
    // twin target critics on (s', a'), then y = r + gamma * min(q1', q2') * (1 - done), kept in
    // the row's thread
    const L0Pre l0_ct2 = load_l0<NT>(a.critic_t[1]);
    fwd_net<NT, RT, kPfWide, 4>(a.critic_t[0], act, stage, xin, red, nullptr, n_rt, nullptr, 0u, row0, B, rt0, top,
                    9, &l0_ct1);
    if (tid < TM) qv[tid] = out_y<RT>(a.critic_t[0], red, tid, 0);
    int q0;  // the first online critic of the block
    if constexpr (POP) q0 = pv.split_twins ? (int)blockIdx.y : 0;
    else q0 = a.split_twins ? (int)blockIdx.y : 0;
    L0Pre l0_on = load_l0<NT>(a.critic[q0]);
    fwd_net<NT, RT, kPfWide, 4>(a.critic_t[1], act, stage, xin, red, nullptr, n_rt, nullptr, 0u, row0, B, rt0, top,
                    15, &l0_ct2);
    float yt = 0.f;
    if (tid < TM) {
        const float q2 = out_y<RT>(a.critic_t[1], red, tid, 0);
        const float rw = brow[tid * 8 + 4], dn = brow[tid * 8 + 7];
        yt = rw + (a.gamma * fminf(qv[tid], q2)) * (1.0f - dn);
        *reinterpret_cast<float4*>(xin + tid * 4) = *reinterpret_cast<const float4*>(brow + tid * 8);
    }
    __syncthreads();
    NAV_MARK(21);
    // online critics on (s, a): both, or (split_twins) the one of this workgroup's grid row
#pragma unroll 1
    for (int q = 0; q < 2; ++q) {
        if constexpr (POP) {
            if (pv.split_twins && q != (int)blockIdx.y) continue;
        } else {
            if (a.split_twins && q != (int)blockIdx.y) continue;  // workgroup-uniform
        }
        uint32_t top_bits[RT * 2];
        WoCols wo;
        fwd_net<NT, RT, kPfWide, 4>(a.critic[q], act, stage, xin, red, a.masks[q], n_rt, a.acts[q], a.save_mask, row0,
                        B, rt0, top, 22 + 14 * q, &l0_on, top_bits, &wo);
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
        if constexpr (POP) {
            if (q == 0 && !pv.split_twins) l0_on = load_l0<NT>(a.critic[1]);
        } else {
            if (q == 0 && !a.split_twins) l0_on = load_l0<NT>(a.critic[1]);
        }
        float* es = a.eslab[q] ? a.eslab[q] + (int64_t)blockIdx.x * a.ecount : nullptr;
        if constexpr (WEIGHTED)
            loss_epilogue<NT, RT, true>(a.critic[q], top, red, row0, B, yt, a.norm, a.dq[q],
                                        a.loss_part[q] + blockIdx.x, es, px.w, px.td_abs[q]);
        else
            loss_epilogue<NT, RT>(a.critic[q], top, red, row0, B, yt, a.norm, a.dq[q],
                                  a.loss_part[q] + blockIdx.x, es);
        __syncthreads();
        NAV_MARK(28 + 14 * q);
        if (a.row_backward) {
            if (tid < TM)
                *reinterpret_cast<float4*>(dys + tid * 4) =
                    make_float4(red[kWaves * TM + tid], 0.f, 0.f, 0.f);  // loss_epilogue's dq
            __syncthreads();
            bwd_net<NT, RT, kPfWide, CBM>(a.critic[q], act, stage, dys, xin, a.masks[q], n_rt, es, nullptr, a.dz[q],
                            a.dz_save_mask, row0, B, rt0, 29 + 14 * q, top_bits, &wo, false);
            __syncthreads();  // the next forward's layer 0 overwrites the rows
        }
        NAV_MARK(35 + 14 * q);
    }
    NAV_CLOCK(0, 1);
