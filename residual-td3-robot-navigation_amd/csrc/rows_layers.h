// rows_layers.h — one network's pass over a block of rows: the layer epilogues around the GEMMs
// of rows_gemm.h, the forward fwd_net and the row backward bwd_net (the residual-TD3 actor /
// critic MLPs, robot.py:128-206). The thin input layer (K = d_in <= 4) and the bias run on f32
// MFMA (layer0_unit's fma chain bit for bit), the output layer (N = 1 or 2) on the VALU with a
// lane-transpose reduce; ReLU derivatives travel from forward to backward as C-layout bit masks.
// The kernels that call these passes are rows_kernels.h and td3_rows.h; the cross-row weight
// gradients and the reduce + Adam are wgrad.h and reduce_adam.h.
#pragma once
#include "rows_gemm.h"


namespace {

// Store a layer's C-layout result into the LDS rows (the next layer's A operand) and its ReLU
// mask bits; with slots, publish the rows' max |value| for the next GEMM's A scale. Global copies
// of the rows are written afterwards by copy_rows (coalesced).
template <int NT, int RT>
NAV_DEV void store_layer(f32x16 (&acc)[RT][2], float* act, int S_, uint16_t* mask, int64_t rt0,
                         float* slots = nullptr) {
    const int lane = threadIdx.x & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wv);
    float m[RT] = {};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? wc.has0 : wc.has1)) continue;
        const int t = j == 0 ? wc.t0 : wc.t1;
        float* col = act + t * 32 + l32 + 4 * h * S_;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            uint32_t bits = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = acc[rt][j][i];
                col[(rt * 32 + (i & 3) + 8 * (i >> 2)) * S_] = v;
                bits |= pos_bit(v) << i;
                m[rt] = max_nn(m[rt], v);  // post-ReLU: v >= 0
            }
            if (mask) mask[mask_idx(rt0 + rt, NT, t, lane)] = (uint16_t)bits;
        }
    }
    publish_amax(slots, m);
}

// 128 LDS rows -> global [M][hp] rows row0.., float4 per lane (1 KiB per wave instruction).
template <int NT, int RT>
NAV_DEV void copy_rows(const float* act, int S_, float* g, int64_t row0, int64_t M) {
    constexpr int hp = NT * 32, Q4 = hp / 4;
    for (int idx = threadIdx.x; idx < RT * 32 * Q4; idx += kBlock) {
        const int r = idx / Q4, c4 = idx - r * Q4;
        if (row0 + r < M)
            *reinterpret_cast<float4*>(g + (row0 + r) * hp + 4 * c4) =
                *reinterpret_cast<const float4*>(act + r * S_ + 4 * c4);
    }
}

// Edge partials over the block's TM LDS rows, one thread per column n < hp, rows summed in order.
template <int TM>
NAV_DEV void edge_col_sums(const float* act, int S_, int hp, float* out) {
    const int n = threadIdx.x;
    if (n >= hp) return;
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < TM; ++r) s += act[r * S_ + n];
    out[n] = s;
}

// dW0 partial: out[n*d_in + k] = sum_r dz0[r][n] * x[r][k]
template <int TM>
NAV_DEV void edge_w0(const float* act, int S_, int hp, const float* xin, int d_in, float* out) {
    const int n = threadIdx.x;
    if (n >= hp) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
    for (int r = 0; r < TM; ++r) {
        const float g = act[r * S_ + n];
        const float4 x = *reinterpret_cast<const float4*>(xin + 4 * r);
        s0 = fmaf(g, x.x, s0);
        s1 = fmaf(g, x.y, s1);
        s2 = fmaf(g, x.z, s2);
        s3 = fmaf(g, x.w, s3);
    }
    out[n * d_in] = s0;
    if (d_in > 1) out[n * d_in + 1] = s1;
    if (d_in > 2) out[n * d_in + 2] = s2;
    if (d_in > 3) out[n * d_in + 3] = s3;
}

// output j of block row rloc from fwd_net's per-wave partial sums, added in wave order
template <int RT>
NAV_DEV float out_y(const MlpDev& net, const float* red, int rloc, int j) {
    constexpr int TM = RT * 32;
    float y = 0.f;
#pragma unroll
    for (int p = 0; p < kWaves; ++p) y += red[(j * kWaves + p) * TM + rloc];
    return y + net.params[net.b_off[net.n_hidden] + j];
}

// Block row of C-layout element i of row tile rt in lane half h.
NAV_DEV int c_row(int rt, int i, int h) { return rt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h; }

// ReLU mask words of a layer from its C-layout registers (store_layer's bits without the rows).
template <int NT, int RT>
NAV_DEV void store_mask(const f32x16 (&acc)[RT][2], uint16_t* mask, int64_t rt0) {
    const int lane = threadIdx.x & 63;
    const WaveCols<NT> wc(wave_id());
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? wc.has0 : wc.has1)) continue;
        const int t = j == 0 ? wc.t0 : wc.t1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            uint32_t bits = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) bits |= pos_bit(acc[rt][j][i]) << i;  // post-ReLU
            mask[mask_idx(rt0 + rt, NT, t, lane)] = (uint16_t)bits;
        }
    }
}

// Output layer (N = d_out <= 2) straight from the top hidden layer's C-layout registers: every
// lane forms, per block row it holds, the dot product of its (up to) 2 columns with Wo; a
// transpose-reduce across the 32 lanes of each lane half (5 xor exchanges that each halve the
// list a lane carries: 31 exchanges for RT = 2) sums the columns of the wave; the 4 waves'
// partials meet in LDS (red [d_out][4][TM]) and out_y adds them in wave order. No LDS copy of the
// top layer, no barrier between the last GEMM and the output layer. The exchanges run in lane-
// mask order 1, 2, 4, 8, 16, so the big early stages are DPP moves inside a 16-lane row (xor 1 /
// 2: quad_perm, xor 4: half-row mirror then quad_perm, xor 8: row rotate by 8) and only the last,
// single-element one crosses rows (ds_bpermute).

// one halving stage of the transpose-reduce: lanes with bit M_ set keep the upper half of the
// list (n entries) and send the lower half to lane ^ M_
template <int M_, int N_>
NAV_DEV void halve(float* v, int l32) {
    const uint32_t um = (l32 & M_) ? 0xffffffffu : 0u;
    // bitwise selects: a ?: over the list would be turned into a dynamic array index
#pragma unroll
    for (int k = 0; k < N_ / 2; ++k) {
        const uint32_t lo = __float_as_uint(v[k]), hi = __float_as_uint(v[k + N_ / 2]);
        const float send = __uint_as_float((lo & um) | (hi & ~um));
        const float keep = __uint_as_float((hi & um) | (lo & ~um));
        v[k] = keep + lane_xor<M_>(send);
    }
}
// Wo entries of the lane's columns (0 for absent tiles): wo[output][tile]
struct WoCols {
    float w[2][2];
};
template <int NT>
NAV_DEV WoCols load_wo(const MlpDev& net) {
    constexpr int hp = NT * 32;
    const int l32 = threadIdx.x & 31;
    const WaveCols<NT> wc(wave_id());
    const float* Wo = net.params + net.w_off[net.n_hidden];
    const int c0 = wc.t0 * 32 + l32, c1 = (wc.has1 ? wc.t1 : wc.t0) * 32 + l32;
    WoCols r;
#pragma unroll
    for (int jo = 0; jo < 2; ++jo) {
        const bool on = jo < net.d_out;
        r.w[jo][0] = on && wc.has0 ? Wo[jo * hp + c0] : 0.f;
        r.w[jo][1] = on && wc.has1 ? Wo[jo * hp + c1] : 0.f;
    }
    return r;
}

template <int NT, int RT>
NAV_DEV void out_partials(const MlpDev& net, const f32x16 (&top)[RT][2], const WoCols& wo,
                          float* red) {
    // RT = 2 (V = 32): after the 5 halvings lane l32 holds list element bitrev5(l32). RT = 1
    // (V = 16): four halvings leave lanes l32 and l32 ^ 16 with the two halves of element
    // bitrev4(l32 & 15); the fifth exchange adds them and the lane with bit 4 clear writes
    static_assert(RT == 1 || RT == 2, "row tiles per workgroup");
    constexpr int TM = RT * 32, V = RT * 16;
    const int lane = threadIdx.x & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
#pragma unroll
    for (int jo = 0; jo < 2; ++jo) {
        if (jo >= net.d_out) break;
        const float w0 = wo.w[jo][0], w1 = wo.w[jo][1];
        float v[V];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) v[rt * 16 + i] = fmaf(top[rt][1][i], w1, top[rt][0][i] * w0);
        // lane bit b (mask 16 .. 1) picks which half of the list the lane keeps: the survivor k
        // of lane l32 is list element (l32 * KEEP + k)
        halve<1, V>(v, l32);
        halve<2, V / 2>(v, l32);
        halve<4, V / 4>(v, l32);
        halve<8, V / 8>(v, l32);
        if constexpr (V >= 32) {
            halve<16, V / 16>(v, l32);
            const int e = (int)(__builtin_bitreverse32((uint32_t)l32) >> 27);
            red[(jo * kWaves + wv) * TM + c_row(e >> 4, e & 15, h)] = v[0];
        } else {
            v[0] += lane_xor<16>(v[0]);
            if ((l32 & 16) == 0) {
                const int e = (int)(__builtin_bitreverse32((uint32_t)l32) >> 28);
                red[(jo * kWaves + wv) * TM + c_row(0, e, h)] = v[0];
            }
        }
    }
}

// Output-layer weight-gradient partials dWo[jo][c] = sum_rows g[row][jo] * h_top[row][c] of the
// block, straight from the top layer's C-layout registers (g = dL/dy rows in LDS, row stride
// gstride): each lane sums its 16 * RT rows of its columns in (row tile, element) order, then
// the two lane halves (rows +0 / +4) meet by one exchange. bwd_net's h_top path (rows from
// global memory) adds in the same order, so both give the same bits.
template <int NT, int RT>
NAV_DEV void wo_grad_regs(const MlpDev& net, const f32x16 (&top)[RT][2], const float* g,
                          int gstride, float* es) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wave_id());
#pragma unroll
    for (int jo = 0; jo < 2; ++jo) {
        if (jo >= net.d_out) break;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float gv = g[c_row(rt, i, h) * gstride + jo];
                s0 = fmaf(gv, top[rt][0][i], s0);
                s1 = fmaf(gv, top[rt][1][i], s1);
            }
        s0 += __shfl_xor(s0, 32, 64);
        s1 += __shfl_xor(s1, 32, 64);
        if (h == 0) {
            float* o = es + e_wo(net) + jo * net.hp;
            if (wc.has0) o[wc.t0 * 32 + l32] = s0;
            if (wc.has1) o[wc.t1 * 32 + l32] = s1;
        }
    }
}

// OUT_LOSS (d_out = 1): q from the output-layer partials against the TD target yt of the thread's
// row (robot.py:341-345, from the caller), mse_loss's gradient dq = (q - yt) * 2/B, the block's
// sum of (q - y)^2, and the output layer's gradient partials dWo = dq^T h_top, dbo = sum dq while
// h_top is still in LDS. `red` = the [2][PARTS][TM] partial-sum scratch (second half reused).
// WEIGHTED (k_td3_critic_rows_w, prioritised replay): the row's importance weight wrow[r] scales
// dq and the loss term, and |q - yt| goes to td_abs[r]; off, the statements are the plain ones.
template <int NT, int RT, bool WEIGHTED = false>
NAV_DEV void loss_epilogue(const MlpDev& net, const f32x16 (&top)[RT][2], float* red,
                           int64_t row0, int64_t M, float yt, float norm, float* dq,
                           float* loss_slot, float* es, const float* wrow = nullptr,
                           float* td_abs = nullptr) {
    constexpr int TM = RT * 32;
    const int tid = threadIdx.x;
    const int64_t r = row0 + tid;
    float dqv = 0.f, e2 = 0.f;
    if (tid < TM && r < M) {
        const float y = out_y<RT>(net, red, tid, 0);
        const float e = y - yt;
        dqv = e * norm;
        e2 = e * e;
        if constexpr (WEIGHTED) {
            const float wr = wrow[r];
            dqv *= wr;
            e2 *= wr;
            td_abs[r] = fabsf(e);
        }
        dq[r] = dqv;
    }
    float* dqs = red + kWaves * TM;  // [TM] dq (past output 0's partials), then the wave sums
    float* ws = dqs + TM;
    if (tid < TM) dqs[tid] = dqv;
    const float w = wave_sum(e2);
    if ((tid & 63) == 0) ws[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) sum += ws[k];
        *loss_slot = sum;
    }
    if (!es) return;
    wo_grad_regs<NT, RT>(net, top, dqs, 1, es);
    // bo = sum of dq over the block's rows (all in wave 0: TM <= 64), and its 3 padding floats
    if (tid < 64) {
        const float sb = wave_sum(dqv);
        if (tid < 4) es[e_bo(net) + tid] = tid == 0 ? sb : 0.f;
    }
}

// Layer 0's per-lane constants (W0 columns h and 2 + h, the bias) of the wave's column tiles:
// loaded one network pass ahead by the fused row programs, so their latency hides under the
// previous pass instead of opening this pass's layer 0
struct L0Pre {
    float wa[2], wb[2], bias[2];
};
template <int NT>
NAV_DEV L0Pre load_l0(const MlpDev& net) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wave_id());
    const float* W0 = net.params + net.w_off[0];
    const float* b0 = net.params + net.b_off[0];
    const int d_in = net.d_in;
    L0Pre p;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool has = j == 0 ? wc.has0 : wc.has1;
        const int c = (j == 0 ? wc.t0 : wc.t1) * 32 + l32;
        p.wa[j] = has && h < d_in ? W0[c * d_in + h] : 0.f;
        p.wb[j] = has && 2 + h < d_in ? W0[c * d_in + 2 + h] : 0.f;
        p.bias[j] = has ? b0[c] : 0.f;  // the column's bias in both lane halves (the C operand)
    }
    return p;
}

// One network's forward over the block's TM rows (input rows xin [TM][4] in LDS). The top hidden
// layer stays in registers (`top`, C layout) — its LDS rows are written only when save_mask asks
// for its global copy — and the output layer's per-wave partials land in `red` (ready for out_y
// after the trailing barrier).
// DIN: the network's d_in when the caller knows it (2 actor, 4 critic; 0: read net.d_in), so the
// layer-0 product has no branch on the input count
template <int NT, int RT, int PFB = 1, int DIN = 0>
NAV_DEV void fwd_net(const MlpDev& net, float* act, _Float16* stage, const float* xin, float* red,
                     uint16_t* masks, int64_t n_rt, float* act_save, uint32_t save_mask,
                     int64_t row0, int64_t M, int64_t rt0, f32x16 (&top)[RT][2], int mk = -64,
                     const L0Pre* pre = nullptr, uint32_t* top_bits = nullptr,
                     WoCols* wo_out = nullptr) {
    constexpr int hp = NT * 32, SS = hp + 4;
    NAV_MARK(mk);
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int nh = net.n_hidden;
    const WaveCols<NT> wc(wv);
    (void)tid;
    // the output layer's Wo columns: issued now, in flight under layer 0 and the GEMMs
    const WoCols wo = load_wo<NT>(net);
    if (wo_out) *wo_out = wo;
    // ---- layer 0 (K = d_in <= 4) on MFMA, straight into the C layout of the wave's column
    // tiles: the C tile starts at the bias (set by VALU), then x[:, 0:2] and (d_in > 2) x[:, 2:4]
    // against W0's columns: each element is fma(x3, w3, fma(x2, w2, fma(x1, w1, fma(x0, w0, b))))
    // — layer0_unit's chain, bit for bit (absent inputs and weights are 0)
    {
        const L0Pre l0 = pre ? *pre : load_l0<NT>(net);
        float m0[RT] = {};
        const bool x23 = DIN == 0 ? net.d_in > 2 : DIN > 2;
        // A operands: row l32 of each row tile, inputs h and 2 + h
        float xa[RT], xb[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const float4 xr = *reinterpret_cast<const float4*>(xin + (rt * 32 + l32) * 4);
            xa[rt] = h ? xr.y : xr.x;
            xb[rt] = h ? xr.w : xr.z;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!(j == 0 ? wc.has0 : wc.has1)) continue;
            const int t = j == 0 ? wc.t0 : wc.t1;
            const int c = t * 32 + l32;
            const float wa = l0.wa[j], wb = l0.wb[j];
            // the C tile starts at the column's bias, set by VALU (exactly what the K = 2 MFMA of
            // (1, 0) x (b, 0) gave); inputs 2, 3 only for d_in > 2
            f32x16 bias;
#pragma unroll
            for (int i = 0; i < 16; ++i) bias[i] = l0.bias[j];
            float* col = act + c + 4 * h * SS;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                f32x16 v = mfma(xa[rt], wa, bias);
                if (x23) v = mfma(xb[rt], wb, v);
                uint32_t bits = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float r = relu(v[i]);
                    col[(rt * 32 + (i & 3) + 8 * (i >> 2)) * SS] = r;
                    bits |= pos_bit(r) << i;
                    m0[rt] = max_nn(m0[rt], r);
                }
                if (masks) masks[mask_idx(rt0 + rt, NT, t, lane)] = (uint16_t)bits;
            }
        }
        if (nh >= 2) publish_amax(amax_slots<RT * 32>(stage), m0);  // layer 1's A scale
    }
    NAV_MARK(mk + 1);
    __syncthreads();
    NAV_MARK(mk + 2);
    if (act_save && (save_mask & 1u)) copy_rows<NT, RT>(act, SS, act_save, row0, M);
    // one hidden x hidden layer on MFMA: acc = relu(rows . W_L + b_L), C layout
    auto hidden_layer = [&](int L, f32x16 (&acc)[RT][2]) {
        // the bias is loaded before the product so its latency hides under the MFMAs
        const float* bL = net.params + net.b_off[L];
        const float bb0 = wc.has0 ? bL[wc.t0 * 32 + l32] : 0.f;
        const float bb1 = wc.has1 ? bL[wc.t1 * 32 + l32] : 0.f;
        gemm_cols<NT, RT, PFB>(act, SS, img_fwd(net, L), stage, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!(j == 0 ? wc.has0 : wc.has1)) continue;
            const float b = j == 0 ? bb0 : bb1;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[rt][j][i] = relu(acc[rt][j][i] + b);
        }
    };
    auto mask_of = [&](int L) { return masks ? masks + (size_t)L * n_rt * NT * 64 : nullptr; };
    // ---- layers 1 .. nh-2: rows back into LDS for the next layer
    for (int L = 1; L + 1 < nh; ++L) {
        f32x16 acc[RT][2];
        hidden_layer(L, acc);
        NAV_TRACE_MARK(50);
        __syncthreads();  // every wave has finished reading the layer's input rows
        store_layer<NT, RT>(acc, act, SS, mask_of(L), rt0, amax_slots<RT * 32>(stage));
        __syncthreads();
        NAV_TRACE_MARK(51);
        if (act_save && ((save_mask >> L) & 1u))
            copy_rows<NT, RT>(act, SS, act_save + (int64_t)L * M * hp, row0, M);
    }
    // ---- the top hidden layer: registers (defined here only, so they are not live above)
    if (nh >= 2) {
        const int L = nh - 1;
        hidden_layer(L, top);
        NAV_MARK(mk + 3);
        if (act_save && ((save_mask >> L) & 1u)) {
            __syncthreads();
            store_layer<NT, RT>(top, act, SS, mask_of(L), rt0);
            __syncthreads();
            copy_rows<NT, RT>(act, SS, act_save + (int64_t)L * M * hp, row0, M);
        } else if (masks && !top_bits) {
            store_mask<NT, RT>(top, mask_of(L), rt0);
        }
        if (top_bits) {  // the top layer's ReLU bits stay in registers for the row backward
            uint16_t* mk = masks && !(act_save && ((save_mask >> L) & 1u)) ? mask_of(L) : nullptr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool has = j == 0 ? wc.has0 : wc.has1;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    uint32_t bits = 0;
#pragma unroll
                    for (int i = 0; i < 16; ++i) bits |= pos_bit(top[rt][j][i]) << i;  // post-ReLU
                    top_bits[rt * 2 + j] = has ? bits : 0u;
                    if (mk && has)
                        mk[mask_idx(rt0 + rt, NT, j == 0 ? wc.t0 : wc.t1, lane)] = (uint16_t)bits;
                }
            }
        }
    } else {
        // the top layer is layer 0: its C-layout registers from the LDS rows just written
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool has = j == 0 ? wc.has0 : wc.has1;
            const float* col = act + (j == 0 ? wc.t0 : wc.t1) * 32 + l32;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) top[rt][j][i] = has ? col[c_row(rt, i, h) * SS] : 0.f;
        }
    }

    // ---- output layer (N = d_out <= 2) from the registers; a barrier publishes the partials
    out_partials<NT, RT>(net, top, wo, red);
    NAV_MARK(mk + 4);
    __syncthreads();
    NAV_MARK(mk + 5);
}

// ---------------- row-local backward ----------------
// The lane's ReLU mask words of one layer (issued ahead of the product that needs them).
template <int NT, int RT>
NAV_DEV void load_mask_bits(const uint16_t* mask, int64_t rt0, uint32_t (&bits)[RT][2]) {
    const int lane = threadIdx.x & 63;
    const WaveCols<NT> wc(wave_id());
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool has = j == 0 ? wc.has0 : wc.has1;
        const int t = j == 0 ? wc.t0 : wc.t1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) bits[rt][j] = has ? mask[mask_idx(rt0 + rt, NT, t, lane)] : 0u;
    }
}

// Edge partials of one hidden layer's dz from the C-layout registers: db[c] = column sum over the
// block's rows (each lane sums its 16 * RT rows in (row tile, element) order, then the two lane
// halves meet: rows +0 / +4), and for layer 0 also dW0[c][k] = sum_rows dz[row][c] x[row][k]
// (x rows from xin [TM][4], one broadcast read per row shared by both column tiles).
template <int NT, int RT>
NAV_DEV void edge_regs(const MlpDev& net, const f32x16 (&z)[RT][2], const float* xin, int L,
                       float* es) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wave_id());
    const int d_in = net.d_in;
    float sb[2] = {0.f, 0.f}, sw[2][4] = {};
    if (L == 0) {
        // dW0's four input columns as two packed pairs (v_pk_fma_f32: the same fused op per
        // element as fmaf, two elements per instruction)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 w01[2] = {{0.f, 0.f}, {0.f, 0.f}}, w23[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float4 x = *reinterpret_cast<const float4*>(xin + c_row(rt, i, h) * 4);
                const f32x2 x01 = {x.x, x.y}, x23 = {x.z, x.w};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float v = z[rt][j][i];
                    const f32x2 vv = {v, v};
                    sb[j] += v;
                    w01[j] = __builtin_elementwise_fma(vv, x01, w01[j]);
                    w23[j] = __builtin_elementwise_fma(vv, x23, w23[j]);
                }
            }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            sw[j][0] = w01[j].x; sw[j][1] = w01[j].y; sw[j][2] = w23[j].x; sw[j][3] = w23[j].y;
        }
    } else {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) sb[j] += z[rt][j][i];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        sb[j] += __shfl_xor(sb[j], 32, 64);
        if (L == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) sw[j][k] += __shfl_xor(sw[j][k], 32, 64);
    }
    if (h != 0) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? wc.has0 : wc.has1)) continue;
        const int c = (j == 0 ? wc.t0 : wc.t1) * 32 + l32;
        es[e_b(net, L) + c] = sb[j];
        if (L == 0)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < d_in) es[net.w_off[0] + c * d_in + k] = sw[j][k];
    }
}

// Masks the layer's dz registers in place (ReLU derivative bits), without the LDS rows.
template <int NT, int RT>
NAV_DEV void mask_regs(f32x16 (&acc)[RT][2], const uint32_t (&mbits)[RT][2]) {
    const WaveCols<NT> wc(wave_id());
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool has = j == 0 ? wc.has0 : wc.has1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                acc[rt][j][i] = has && ((mbits[rt][j] >> i) & 1u) ? acc[rt][j][i] : 0.f;
    }
}

// Masks the layer's dz registers in place (ReLU derivative bits) and stores them to the LDS rows;
// with slots, publishes their max |value| for the next GEMM's A scale.
template <int NT, int RT>
NAV_DEV void mask_and_store(f32x16 (&acc)[RT][2], const uint32_t (&mbits)[RT][2], float* act,
                            int S_, float* slots = nullptr) {
    const int lane = threadIdx.x & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wv);
    float m[RT] = {};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!(j == 0 ? wc.has0 : wc.has1)) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[rt][j][i] = 0.f;
            continue;
        }
        const int t = j == 0 ? wc.t0 : wc.t1;
        float* col = act + t * 32 + l32 + 4 * h * S_;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint32_t bits = mbits[rt][j];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc[rt][j][i] = (bits >> i) & 1u ? acc[rt][j][i] : 0.f;
                col[(rt * 32 + (i & 3) + 8 * (i >> 2)) * S_] = acc[rt][j][i];
                m[rt] = fmaxf(m[rt], fabsf(acc[rt][j][i]));
            }
        }
    }
    publish_amax(slots, m);
}

// One network's row backward over the block's TM rows: dy rows in dys [TM][4] (LDS, ready), the
// forward's ReLU bits in masks; leaves dz_0 in the LDS rows `act`. With es: the per-block edge
// partials (every bias, dW0 from the input rows xin [TM][4], and dWo / dbo when h_top [M][hp] is
// given); dz_L rows to dz for save_mask bits.
// BM: the top layer's product form. 0: every layer on gemm_cols (any d_out); 1: d_out = 1, the
// top layer on gemm_bits, the layers below on gemm_cols (n_hidden >= 3); 2: d_out = 1 and
// n_hidden = 2, gemm_bits only. Compile-time, so a kernel carries only the forms it runs (both
// forms in one function took the row kernels past 256 registers: one workgroup per CU).
template <int NT, int RT, int PFB = 1, int BM = 0>
NAV_DEV void bwd_net(const MlpDev& net, float* act, _Float16* stage, const float* dys, const float* xin,
                     const uint16_t* masks, int64_t n_rt, float* es, const float* h_top,
                     float* dz, uint32_t save_mask, int64_t row0, int64_t M, int64_t rt0,
                     int mk = -64, const uint32_t* top_bits = nullptr,
                     const WoCols* wo_in = nullptr, bool dz0_rows = true) {
    constexpr int hp = NT * 32, SS = hp + 4, TM = RT * 32;
    NAV_MARK(mk);
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const int d_in = net.d_in, d_out = net.d_out, nh = net.n_hidden;
    const int64_t MH = M * hp;
    const WaveCols<NT> wc(wv);
    const size_t mstride = (size_t)n_rt * NT * 64;
    if (es) {
        // output layer (robot.py:361 / 392 backward): dWo = dy^T h_top, dbo = sum dy, when the
        // forward did not produce them (it does for the critic's TD loss)
        if (h_top) {
            // rows in wo_grad_regs' order: per lane half, (row tile, C element); halves added last
            const int n = tid;
            if (n < hp) {
                float s0[2] = {0.f, 0.f}, s1[2] = {0.f, 0.f};
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll 4
                        for (int i = 0; i < 16; ++i) {
                            const int rr = c_row(rt, i, hh);
                            if (row0 + rr >= M) continue;
                            const float hv = h_top[(row0 + rr) * hp + n];
                            s0[hh] = fmaf(dys[rr * 4], hv, s0[hh]);
                            s1[hh] = fmaf(dys[rr * 4 + 1], hv, s1[hh]);
                        }
                es[e_wo(net) + n] = s0[0] + s0[1];
                if (d_out > 1) es[e_wo(net) + hp + n] = s1[0] + s1[1];
            }
            if (tid < 4) {
                float s = 0.f;
                if (tid < d_out)
                    for (int rr = 0; rr < TM; ++rr) s += dys[rr * 4 + tid];
                es[e_bo(net) + tid] = s;
            }
        }
    }

    // d_out = 1: the top layer's backward product runs on the forward's ReLU bits (gemm_bits; the
    // Wt image is the only backward image of that layer); its dz rows are still formed (and
    // copied out) where save_mask asks for them
    constexpr bool bits_path = BM > 0;
    const bool save_top = (save_mask >> (nh - 1)) & 1u;
    // top hidden layer: dz = (dy . Wo) * relu'(.), in the C layout: one K = 2 MFMA per tile of
    // dy rows (lane l32 = row, h = output) against Wo's columns, fma(dy1, w1, dy0 w0) — the
    // chain the weight-gradient kernel recomputes — then the forward's ReLU bits. On the bits
    // path these registers only feed the layer's bias partials (and are skipped without es).
    uint32_t mb[RT][2];
    {
        const float* Wo = net.params + net.w_off[nh];
        const uint16_t* mk = masks + (size_t)(nh - 1) * mstride;
        const f32x16 zero = {};
        float ga[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const float4 g = *reinterpret_cast<const float4*>(dys + (rt * 32 + l32) * 4);
            ga[rt] = h < d_out ? (h ? g.y : g.x) : 0.f;
        }
        if (top_bits) {  // the forward's bits of this top layer, still in registers
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int j = 0; j < 2; ++j) mb[rt][j] = top_bits[rt * 2 + j];
        } else {
            load_mask_bits<NT, RT>(mk, rt0, mb);
        }
        if (!bits_path || (es && nh > 1) || save_top) {
            f32x16 z[RT][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool has = j == 0 ? wc.has0 : wc.has1;
                const int c = (j == 0 ? wc.t0 : has ? wc.t1 : wc.t0) * 32 + l32;
                // the forward's Wo registers: wo.w[output][tile] holds Wo[output][c] (0 when absent)
                const float wb = wo_in ? (h ? wo_in->w[1][j] : wo_in->w[0][j])
                                       : has && h < d_out ? Wo[h * hp + c] : 0.f;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) z[rt][j] = mfma(ga[rt], wb, zero);
            }
            if (bits_path && !save_top)
                mask_regs<NT, RT>(z, mb);
            else
                mask_and_store<NT, RT>(z, mb, act, SS,
                                       !bits_path && nh > 1 ? amax_slots<TM>(stage) : nullptr);
            if (es && nh > 1) edge_regs<NT, RT>(net, z, xin, nh - 1, es);
        }
        if (bits_path) {
            if (save_top) {  // the top layer's dz rows themselves, before the scratch reuses act
                __syncthreads();
                copy_rows<NT, RT>(act, SS, dz + (int64_t)(nh - 1) * MH, row0, M);
                __syncthreads();
            }
            bits_stage<NT, RT>(act, mb, dys);
        }
    }
    NAV_MARK(mk + 1);
    __syncthreads();
    // per layer: the rows themselves only where the weight-gradient kernel cannot recompute them
    // (save_mask); the edge partials come from the registers (edge_regs), except for a one-layer
    // network's layer 0 written by the top unit above (LDS column sums)
    auto finish_layer = [&](int L) {
        if (es && nh == 1) {
            edge_col_sums<TM>(act, SS, hp, es + e_b(net, L));
            edge_w0<TM>(act, SS, hp, xin, d_in, es + net.w_off[0]);
        }
        if ((save_mask >> L) & 1u) copy_rows<NT, RT>(act, SS, dz + (int64_t)L * MH, row0, M);
    };
    if (!bits_path) finish_layer(nh - 1);
    NAV_MARK(mk + 2);

    // after layer L's product (acc = dz_L . W_L): mask with layer L - 1's bits, its rows to LDS
    // where a reader follows, its edge partials
    auto after_product = [&](int L, f32x16 (&acc)[RT][2], const uint32_t (&mbits)[RT][2]) {
        __syncthreads();
        // layer 0's rows only when a reader follows (the caller's dx, the save copy); its edge
        // partials come from the registers
        if (L > 1 || dz0_rows || (save_mask & 1u))
            mask_and_store<NT, RT>(acc, mbits, act, SS, L > 1 ? amax_slots<TM>(stage) : nullptr);
        else
            mask_regs<NT, RT>(acc, mbits);
        if (es) edge_regs<NT, RT>(net, acc, xin, L - 1, es);
        __syncthreads();
        NAV_MARK(mk + 4);
        finish_layer(L - 1);
    };
    int Ltop = nh - 1;
    if (bits_path) {
        f32x16 acc[RT][2];
        uint32_t mbits[RT][2];
        load_mask_bits<NT, RT>(masks + (size_t)(nh - 2) * mstride, rt0, mbits);
        gemm_bits<NT, RT, PFB>(act, img_bwd(net, nh - 1), acc);
        NAV_MARK(mk + 3);
        after_product(nh - 1, acc, mbits);
        Ltop = nh - 2;
    }
    // hidden layers, top-down: dz_{L-1} = (dz_L . W_L) * relu'(act_{L-1}), B = packed Wb_L
    if constexpr (BM != 2) {
        for (int L = Ltop; L >= 1; --L) {
            f32x16 acc[RT][2];
            uint32_t mbits[RT][2];
            load_mask_bits<NT, RT>(masks + (size_t)(L - 1) * mstride, rt0, mbits);
            gemm_cols<NT, RT, PFB>(act, SS, img_bwd(net, L), stage, acc);
            NAV_MARK(mk + 3);
            after_product(L, acc, mbits);
        }
    }
    NAV_MARK(mk + 5);

}

// dL/dx[row][jj] = dz_0[row] . W0[:, jj] from the LDS rows (after bwd_net)
template <int NT>
NAV_DEV float dx_unit(const MlpDev& net, const float* act, int rloc, int jj) {
    constexpr int hp = NT * 32, SS = hp + 4;
    const float* W0 = net.params + net.w_off[0];
    const float* zr = act + rloc * SS;
    float acc = 0.f;
    for (int c = 0; c < hp; ++c) acc = fmaf(zr[c], W0[c * net.d_in + jj], acc);
    return acc;
}

}  // namespace
