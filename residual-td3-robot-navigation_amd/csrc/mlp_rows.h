// mlp_rows.h — the device code of the row kernels: the residual-TD3 actor/critic MLPs
// (robot.py:128-206) and their learner (robot.py:209-398) on gfx950.
//
// Forward / row-backward: one 256-thread workgroup = 4 waves = a block of 64 rows (32 for small
// batches) kept in LDS as fp32 (row stride hp+4) across all layers. Hidden x hidden layers run on
// the fp16 matrix cores (v_mfma_f32_32x32x16_f16) at f32-class accuracy: each fp32 operand is
// scaled by a power of two (A per 32-row tile, B per column) and split into two fp16 planes
// (hi + lo carries 22 significant bits), and the three products lo.hi + hi.lo + hi.hi accumulate
// in fp32 (mlp_common.h; tests/test_gpu_mlp.py pins the result against an fp64 reference at 2e-6
// of scale). Every wave owns 1-2 32-column tiles of all the block's rows; the A operand is split
// once per k step into an LDS stage shared by the 4 waves, the B operand streams from the
// L2-resident split weight image (refreshed after Adam / Polyak). The thin input layer (K = d_in
// <= 4) and the bias run on f32 MFMA (layer0_unit's fma chain bit for bit), the output layer (N =
// 1 or 2) on the VALU with a lane-transpose reduce; ReLU derivatives travel from forward to
// backward as C-layout bit masks. The cross-row weight
// gradients and the reduce + Adam are wgrad.h and reduce_adam.h. The per-width launchers are
// mlp_rows_nt.hip, the C ABI is mlp_abi.hip: nothing host-side here but sizes and argument
// structs.
#pragma once
#include "mlp_common.h"
#include "nav_tick.h"


namespace {

// B-fragment prefetch distance (k steps) of the 64-row GEMMs in the critic row kernel and the
// forward / tick kernels (the actor row kernel keeps 1: profiles/r05aq)
constexpr int kPfWide = 2;

template <int NT>
struct WaveCols {
    int t0, t1;
    bool has0, has1;
    NAV_DEV WaveCols(int wv) : t0(wv), t1(wv + 4), has0(NT >= 4 || wv < NT), has1(NT >= 8 || wv + 4 < NT) {}
};

// Per-(32-row tile, wave) max |value| slots of the block (float[RT][kWaves], just past gemm_cols'
// split stage): the epilogue that writes a GEMM's A rows into LDS publishes its values' max per
// row tile here, and gemm_cols reads them (after the epilogue's barrier) for the A operand's
// power-of-two scale of each 32-row tile. Per row tile, not per workgroup: 32- and 64-row blocks
// then scale every row identically, so the forward stays bit-identical across block heights.
template <int TM>
NAV_DEV float* amax_slots(_Float16* stage);
NAV_DEV _Float16* whole_stage(_Float16* stage);

template <int RT>
NAV_DEV void publish_amax(float* slots, const float (&m)[RT]) {
    if (!slots) return;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const float v = wave_max_abs(m[rt]);
        if ((threadIdx.x & 63) == 0) slots[rt * kWaves + (threadIdx.x >> 6)] = v;
    }
}

constexpr int kPF1 = 2;  // B prefetch distance of 32-row blocks

// gemm_cols for 32-row blocks (small batches, latency-bound): the workgroup scales and splits
// the whole layer's 32 x hp A values into the whole-layer stage at once (two k steps per pass of
// the block, the same per-step layout and swizzle as the stage below), passes ONE barrier, and
// every wave then runs all k steps from LDS with no barrier in the product; the per-step stage
// cost a barrier + fragment-read round trip per k step (~640 cycles per step at hp = 224 vs the
// step's 6 MFMAs, profiles/r06x). Same products, same order: bit-identical to the per-step form.
template <int NT>
NAV_DEV void gemm_cols_whole(const float* __restrict__ A, int S_, const float* __restrict__ img,
                             _Float16* stage, f32x16 (&acc)[1][2]) {
    constexpr int hp = NT * 32;
    constexpr int nq = hp / 16;
    constexpr size_t PL = (size_t)nq * 2 * hp;
    constexpr size_t STEP = 2 * (size_t)hp;
    constexpr int PP = 32 * 16;  // fp16 per plane per step
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wv);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[0][j][i] = 0.f;
    const int t0 = wc.has0 ? wc.t0 : 0, t1 = wc.has1 ? wc.t1 : t0;
    const float* sl = amax_slots<32>(stage);
    const int ea = pow2_exp(fmaxf(fmaxf(sl[0], sl[1]), fmaxf(sl[2], sl[3])));
    const int* ex = image_exps(img, hp);
    const int eb0 = ex[t0 * 32 + l32], eb1 = ex[t1 * 32 + l32];
    const char* Bb = reinterpret_cast<const char*>(img);
    const uint32_t o0 = (uint32_t)(h * hp + t0 * 32 + l32) * 16u;
    const uint32_t o1 = (uint32_t)(h * hp + t1 * 32 + l32) * 16u;
    auto ldB = [&](uint32_t o, int p, int q) {
        return *reinterpret_cast<const f16x8*>(Bb + (o + (uint32_t)((p * PL + q * STEP) * 16)));
    };
    constexpr int PF = kPF1 < nq ? kPF1 : nq;
    f16x8 bq0[PF + 1][2], bq1[PF + 1][2];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            bq0[d][p] = ldB(o0, p, d);
            bq1[d][p] = ldB(o1, p, d);
        }
    // the split: thread (step parity qo, row sr, k offset sk) takes 4 values of steps qo, qo + 2, ..
    _Float16* const whole = whole_stage(stage);
    const int qo = tid >> 7, sr = (tid >> 2) & 31, sk = (tid & 3) * 4;
    const float* src = A + sr * S_ + sk + 16 * qo;
    _Float16* dst = whole + qo * 2 * PP + sr * 16 + ((((sk >> 3) ^ (sr >> 3)) & 1) << 3) + (sk & 7);
    const float sa = ldexpf(1.f, ea);
    float4 xs[nq / 2];
#pragma unroll
    for (int p = 0; p < nq / 2; ++p) xs[p] = *reinterpret_cast<const float4*>(src + 32 * p);
#pragma unroll
    for (int p = 0; p < nq / 2; ++p) {
        const float v[4] = {xs[p].x * sa, xs[p].y * sa, xs[p].z * sa, xs[p].w * sa};
        f16x4 ph, pl;
#pragma unroll
        for (int j = 0; j < 4; ++j) ph[j] = (_Float16)v[j];
        pin_value(ph);  // lo from the stored hi's bits (mlp_common.h)
#pragma unroll
        for (int j = 0; j < 4; ++j) pl[j] = (_Float16)(v[j] - (float)ph[j]);
        *reinterpret_cast<f16x4*>(dst + p * 4 * PP) = ph;
        *reinterpret_cast<f16x4*>(dst + p * 4 * PP + PP) = pl;
    }
    __syncthreads();
    const _Float16* frag = whole + l32 * 16 + (((h ^ (l32 >> 3)) & 1) << 3);
    auto ldA = [&](int q) {
        Split2 a;
        a.h = *reinterpret_cast<const f16x8*>(frag + q * 2 * PP);
        a.l = *reinterpret_cast<const f16x8*>(frag + q * 2 * PP + PP);
        return a;
    };
    Split2 af = ldA(0);
#pragma unroll
    for (int q = 0; q < nq; ++q) {
        if (q + PF < nq) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                bq0[(q + PF) % (PF + 1)][p] = ldB(o0, p, q + PF);
                bq1[(q + PF) % (PF + 1)][p] = ldB(o1, p, q + PF);
            }
        }
        Split2 an;
        if (q + 1 < nq) an = ldA(q + 1);
        if (wc.has0) {  // wave-uniform
            acc[0][0] = mfma_x3(af, bq0[q % (PF + 1)], acc[0][0]);
            if (NT >= 8 || wc.has1) acc[0][1] = mfma_x3(af, bq1[q % (PF + 1)], acc[0][1]);
        }
        if (q + 1 < nq) af = an;
        // a scheduling fence per k step (as in gemm_bits): without a barrier in the loop the
        // scheduler sinks the prefetched loads down to their uses
        __builtin_amdgcn_sched_barrier(0);
    }
    const int u0 = -(ea + eb0), u1 = -(ea + eb1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[0][0][i] = ldexpf(acc[0][0][i], u0);
        acc[0][1][i] = ldexpf(acc[0][1][i], u1);
    }
}

// acc[rt][j] = A[TM rows][hp] (LDS f32, row stride S_) x B[hp][tile t_j] on the fp16 matrix
// cores at f32 accuracy (mlp_common.h: power-of-two scales, two-plane fp16 split, three
// products). Per 16-deep k step the workgroup scales and splits the step's TM x 16 A values ONCE,
// four per thread, into an LDS stage of two fp16 planes (split_stage), and every wave reads its
// 16-B fragments from there (before: each of the 4 waves split every A value it read — the split
// was ~15 % of the GEMM; probe r03v: -10 %). Two barriers per step: stage written, stage read. B is
// the layer's image (split_entry layout, per-column exponents after the planes) in global
// memory, L2-resident, its two planes loaded PF steps ahead. Lane (h, l32) holds A[row
// l32][16q + 8h + j] and B[16q + 8h + j][col l32], j = 0..7 (the 32x32x16 operand maps). Every wave
// runs the split and the barriers; waves without a column tile (NT < 4) skip only the MFMAs. The
// result is unscaled before it is returned: the callers see acc = A . B in f32.
template <int NT, int RT, int PF>
NAV_DEV void gemm_cols_step(const float* __restrict__ A, int S_, const float* __restrict__ img,
                            _Float16* stage, f32x16 (&acc)[RT][2]) {
    static_assert(RT == 2, "the 64-row form only: 32-row blocks take gemm_cols_whole");
    constexpr int hp = NT * 32;
    constexpr int nq = hp / 16;
    constexpr int TM = RT * 32;
    constexpr size_t PL = (size_t)nq * 2 * hp;  // 16-B entries per plane
    constexpr size_t STEP = 2 * (size_t)hp;     // entries per k step
    constexpr int PP = TM * 16;                 // fp16 per stage plane
    const int tid = threadIdx.x, lane = tid & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wv);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][j][i] = 0.f;
    // A wave without a second tile re-reads its first tile's B (same cache lines) so every load
    // is unconditional; its second-tile MFMAs are skipped by a scalar branch (a wave without any
    // tile reads tile 0's and issues none).
    const int t0 = wc.has0 ? wc.t0 : 0, t1 = wc.has1 ? wc.t1 : t0;
    // the scales: A's per 32-row tile from the producing epilogue's published maxima, B's per
    // column (in flight under the whole product)
    const float* slots = amax_slots<TM>(stage);
    int ea[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const float* sl = slots + rt * kWaves;
        ea[rt] = pow2_exp(fmaxf(fmaxf(sl[0], sl[1]), fmaxf(sl[2], sl[3])));
    }
    const int* ex = image_exps(img, hp);
    const int eb0 = ex[t0 * 32 + l32], eb1 = ex[t1 * 32 + l32];
    // B entries as the uniform image base + a 32-bit per-lane byte offset (SGPR base + VGPR
    // offset addressing: one 32-bit add per load instead of a 64-bit address pair)
    const char* Bb = reinterpret_cast<const char*>(img);
    const uint32_t o0 = (uint32_t)(h * hp + t0 * 32 + l32) * 16u;
    const uint32_t o1 = (uint32_t)(h * hp + t1 * 32 + l32) * 16u;
    auto ldB = [&](uint32_t o, int p, int q) {
        return *reinterpret_cast<const f16x8*>(Bb + (o + (uint32_t)((p * PL + q * STEP) * 16)));
    };
    // B planes PF steps ahead, the caller's choice: 2 in the critic row kernel and the forward /
    // tick launches, 1 in the 256-register actor row kernel, where a second step of B fragments
    // costs more than it hides (profiles/r05ap)
    f16x8 bq0[PF + 1][2], bq1[PF + 1][2];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int qd = d < nq ? d : nq - 1;
            bq0[d][p] = ldB(o0, p, qd);
            bq1[d][p] = ldB(o1, p, qd);
        }
    // this thread's share of a step: 4 values of row sr at k offset sk; the stage's two 16-B
    // halves of row r are swapped when (r >> 3) & 1, which makes both the 8-B stores and the
    // waves' 16-B fragment reads bank-conflict-free (ds_read_b128 lane groups). With 64 rows
    // every thread has a share (no branch: the split sits in the MFMAs' basic block)
    static_assert(TM * 4 == kBlock, "one share per thread");
    const int sr = tid >> 2, sk = (tid & 3) * 4;
    const float* src = A + sr * S_ + sk;
    _Float16* dst = stage + sr * 16 + ((((sk >> 3) ^ (sr >> 3)) & 1) << 3) + (sk & 7);
    const _Float16* frag = stage + l32 * 16 + (((h ^ (l32 >> 3)) & 1) << 3);
    float4 x = *reinterpret_cast<const float4*>(src);
    const float sa = ldexpf(1.f, ea[(sr >> 5) < RT ? (sr >> 5) : RT - 1]);
    // scale + split of step q's share (x) into the stage, the next x from the LDS rows, B planes
    // ahead
    auto produce = [&](int q) {
        const float v[4] = {x.x * sa, x.y * sa, x.z * sa, x.w * sa};
        f16x4 ph, pl;
#pragma unroll
        for (int j = 0; j < 4; ++j) ph[j] = (_Float16)v[j];
        pin_value(ph);  // lo from the stored hi's bits (mlp_common.h)
#pragma unroll
        for (int j = 0; j < 4; ++j) pl[j] = (_Float16)(v[j] - (float)ph[j]);
        *reinterpret_cast<f16x4*>(dst) = ph;
        *reinterpret_cast<f16x4*>(dst + PP) = pl;
        if (q + 1 < nq) x = *reinterpret_cast<const float4*>(src + 16 * (q + 1));
        // production of step q runs during step q - 1's MFMAs: the B planes loaded here are
        // step q - 1 + PF's (steps 0 .. PF - 1 come from the prologue)
        const int qb = q - 1 + PF;
        if (q >= 1 && qb < nq) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                bq0[qb % (PF + 1)][p] = ldB(o0, p, qb);
                bq1[qb % (PF + 1)][p] = ldB(o1, p, qb);
            }
        }
    };
    Split2 sa2[RT];
    // two barriers per step: the stage is written, then read (the next step may overwrite it)
    auto consume = [&]() {
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const _Float16* f = frag + rt * 32 * 16;
            sa2[rt].h = *reinterpret_cast<const f16x8*>(f);
            sa2[rt].l = *reinterpret_cast<const f16x8*>(f + PP);
        }
        __syncthreads();
    };
    produce(0);
    consume();
    // Two workgroups share a CU at the bench shapes (blocks b and b + kCUs, dispatched together),
    // and at equal priority the SIMD arbiter issues the older wave first: the second workgroup's
    // GEMMs lag and it ends its last ~50 k cycles alone at the lone-workgroup MFMA rate (critic_rows:
    // 247 k vs 297 k cycles). The younger partner of each pair (odd multiples of kCUs) raises its
    // wave priority inside its GEMMs, which balances the pair (270 k / 267 k; critic_rows 161.6 ->
    // 153.5 us, profiles/r04y, r04z). At a 512-block grid this is the grid's upper half.
    const bool favored = (blockIdx.x / kCUs) & 1;
    if (favored) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int q = 0; q < nq; ++q) {
        // step q + 1's production comes first in program order, so the scheduler can place it
        // between step q's MFMAs (its stage stores follow step q's second barrier)
        if (q + 1 < nq) produce(q + 1);
        Split2 cur[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) cur[rt] = sa2[rt];
        if (wc.has0) {  // wave-uniform
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                acc[rt][0] = mfma_x3(cur[rt], bq0[q % (PF + 1)], acc[rt][0]);
                if (NT >= 8 || wc.has1)
                    acc[rt][1] = mfma_x3(cur[rt], bq1[q % (PF + 1)], acc[rt][1]);
            }
        }
        if (q + 1 < nq) consume();
    }
    if (favored) __builtin_amdgcn_s_setprio(0);
    // unscale: acc 2^-(ea[rt] + e_n), exact (v_ldexp_f32)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int u0 = -(ea[rt] + eb0), u1 = -(ea[rt] + eb1);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            acc[rt][0][i] = ldexpf(acc[rt][0][i], u0);
            acc[rt][1][i] = ldexpf(acc[rt][1][i], u1);
        }
    }
}

// 32-row blocks take the whole-layer stage, 64-row blocks the per-step stage with the caller's B
// prefetch distance
template <int NT, int RT, int PFB = 1>
NAV_DEV void gemm_cols(const float* __restrict__ A, int S_, const float* __restrict__ img,
                       _Float16* stage, f32x16 (&acc)[RT][2]) {
    if constexpr (RT == 1)
        gemm_cols_whole<NT>(A, S_, img, stage, acc);
    else
        gemm_cols_step<NT, RT, PFB>(A, S_, img, stage, acc);
}

// ---- the top hidden layer's row backward of a d_out = 1 network on its ReLU bits ----
// dz_{L-1}[r][c] = e_{L-1}[r][c] * sum_n dz_L[r][n] W_L[n][c] with dz_L[r][n] = e_L[r][n] g[r]
// Wo[n] (g = dL/dq, e = the forward's ReLU bits) is g[r] * sum_n e_L[r][n] Wt[n][c], Wt[n][c] =
// Wo[n] W_L[n][c]: the A operand is the bit matrix itself, exact in fp16 (0 / 1.0), so only B (the
// Wt image, k_pack_img) is split and each k step takes 2 products instead of 3; no A rows, no
// split stage, no barrier in the product. The bits come row-major from LDS: word w of row r holds
// e_L[r][32 w .. 32 w + 31] (bits_stage), one byte per lane and k step picks a 16-B fragment of
// the 256-entry table of 8 fp16 zeros / ones.
constexpr int kBitTab = 256 * 4;  // floats of the fragment table (256 x 16 B)
// LDS words per row of the bit image: NT + 1 (odd: the 32 lanes of a half read 32 rows without a
// bank conflict)
template <int NT>
constexpr int bit_ws() { return NT + 1; }

// The fragment table (entry b: fp16 bit j of b at element j) and the bit image of the lanes'
// C-layout mask words (mb[rt][j]: bit i = row c_row(rt, i, h), column t_j * 32 + l32) into the
// scratch at `scr` (tab [256][4] u32, then bits [TM][bit_ws] u32, then g [TM]). One ballot per
// (row tile, column tile, C element) yields a row's word for the wave's column tile (lanes h = 0:
// row +0, h = 1: row +4); writelane parks it at the row's lane, lanes 0-31 carry the first tile
// and 32-63 the second, and one store per row tile writes both.
// lane ^ M_ across the wave: DPP moves inside 16-lane rows for M_ <= 8 (out_partials, bits_stage)
template <int M_>
NAV_DEV float lane_xor(float v) {
    const int x = __float_as_int(v);
    if constexpr (M_ == 1) {
        return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false));  // [1,0,3,2]
    } else if constexpr (M_ == 2) {
        return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false));  // [2,3,0,1]
    } else if constexpr (M_ == 4) {
        const int m7 = __builtin_amdgcn_mov_dpp(x, 0x141, 0xF, 0xF, false);  // l ^ 7
        return __int_as_float(__builtin_amdgcn_mov_dpp(m7, 0x1B, 0xF, 0xF, false));  // ^ 3
    } else if constexpr (M_ == 8) {
        return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x128, 0xF, 0xF, false));  // ror 8
    } else {
        return __shfl_xor(v, M_, 64);
    }
}

// one stage of the 32 x 32 bit transpose: lanes l and l ^ S swap the off-diagonal S x S blocks
// (lane_xor: DPP row moves for S <= 8, one ds_bpermute for 16)
template <int S>
NAV_DEV uint32_t bfly_stage(uint32_t x, int lane, uint32_t m) {
    const uint32_t y = __float_as_uint(lane_xor<S>(__uint_as_float(x)));
    return (lane & S) ? (((y >> S) & m) | (x & ~m)) : ((x & m) | ((y & m) << S));
}

template <int NT, int RT>
NAV_DEV void bits_stage(float* scr, const uint32_t (&mb)[RT][2], const float* dys) {
    constexpr int TM = RT * 32, WS = bit_ws<NT>();
    const int tid = threadIdx.x, lane = tid & 63;
    const WaveCols<NT> wc(wave_id());
    static_assert((kBitTab + TM * WS + TM) * 4 <= TM * (NT * 32 + 4) * 4,
                  "the bit scratch fits in the block's LDS rows");
    uint32_t* tab = reinterpret_cast<uint32_t*>(scr);
    uint32_t* bw = tab + kBitTab;
    float* gq = reinterpret_cast<float*>(bw + TM * WS);
    {
        const uint32_t b = (uint32_t)tid;  // kBlock = 256 entries
        uint4 e;
        e.x = ((b & 1u) ? 0x3C00u : 0u) | ((b & 2u) ? 0x3C000000u : 0u);
        e.y = ((b & 4u) ? 0x3C00u : 0u) | ((b & 8u) ? 0x3C000000u : 0u);
        e.z = ((b & 16u) ? 0x3C00u : 0u) | ((b & 32u) ? 0x3C000000u : 0u);
        e.w = ((b & 64u) ? 0x3C00u : 0u) | ((b & 128u) ? 0x3C000000u : 0u);
        reinterpret_cast<uint4*>(tab)[tid] = e;
    }
    if (tid < TM) gq[tid] = dys[tid * 4];
    // per row tile: lanes 0-31 build the column words of the wave's first tile, lanes 32-63 of
    // its second (one exchange across the halves: lane (h, l32) holds rows +4h of both), then a
    // 32 x 32 bit transpose inside each half (5 butterfly exchanges) leaves row l32's word of its
    // half's tile in lane l32. VGPR shuffles only: a ballot form (v_cmp to an SGPR pair, selects
    // on it) gave timing-dependent words in the older workgroup of a co-resident pair
    // (tools/dbg_bits.py, profiles/r06g).
    const int h = lane >> 5;
    auto spread = [](uint32_t w) {  // nibble k of a 16-bit word -> bits 8k .. 8k + 3
        return (w & 0xFu) | ((w & 0xF0u) << 4) | ((w & 0xF00u) << 8) | ((w & 0xF000u) << 12);
    };
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const uint32_t send = h ? mb[rt][0] : mb[rt][1];
        const uint32_t recv = (uint32_t)__shfl_xor((int)send, 32, 64);
        const uint32_t w0 = h ? recv : mb[rt][0], w1 = h ? mb[rt][1] : recv;
        // bit r of x = E[rt * 32 + r][column (tile h) * 32 + l32]
        uint32_t x = spread(w0) | (spread(w1) << 4);
        x = bfly_stage<16>(x, lane, 0x0000FFFFu);
        x = bfly_stage<8>(x, lane, 0x00FF00FFu);
        x = bfly_stage<4>(x, lane, 0x0F0F0F0Fu);
        x = bfly_stage<2>(x, lane, 0x33333333u);
        x = bfly_stage<1>(x, lane, 0x55555555u);
        if (h == 0 ? wc.has0 : wc.has1)
            bw[(rt * 32 + (lane & 31)) * WS + (h == 0 ? wc.t0 : wc.t1)] = x;
    }
}

// acc[rt][j] = g[row] * (E[TM rows][hp] (bit image) x Wt[hp][tile t_j]) from bits_stage's
// scratch and the Wt image (B planes PF steps ahead as in gemm_cols; the A fragments one step
// ahead). Unscaled and multiplied by g[row] before it returns.
template <int NT, int RT, int PFB = 1>
NAV_DEV void gemm_bits(const float* scr, const float* __restrict__ img, f32x16 (&acc)[RT][2]) {
    constexpr int hp = NT * 32;
    constexpr int nq = hp / 16;
    constexpr int TM = RT * 32, WS = bit_ws<NT>();
    constexpr size_t PL = (size_t)nq * 2 * hp;
    constexpr size_t STEP = 2 * (size_t)hp;
    const int lane = threadIdx.x & 63, wv = wave_id(), h = lane >> 5, l32 = lane & 31;
    const WaveCols<NT> wc(wv);
    const uint4* tab = reinterpret_cast<const uint4*>(scr);
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(scr) + kBitTab;
    const float* gq = reinterpret_cast<const float*>(bw + TM * WS);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][j][i] = 0.f;
    // the zero accumulators as registers: folded into an inline-constant C operand, the first
    // product's untied destination was allocated over its own B fragment, and the results came
    // out timing-dependent (a few rows per launch; tools/dbg_bits.py, profiles/r06d)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 2; ++j) pin_value(acc[rt][j]);
    const int t0 = wc.has0 ? wc.t0 : 0, t1 = wc.has1 ? wc.t1 : t0;
    const int* ex = image_exps(img, hp);
    const int eb0 = ex[t0 * 32 + l32], eb1 = ex[t1 * 32 + l32];
    const char* Bb = reinterpret_cast<const char*>(img);
    const uint32_t o0 = (uint32_t)(h * hp + t0 * 32 + l32) * 16u;
    const uint32_t o1 = (uint32_t)(h * hp + t1 * 32 + l32) * 16u;
    auto ldB = [&](uint32_t o, int p, int q) {
        return *reinterpret_cast<const f16x8*>(Bb + (o + (uint32_t)((p * PL + q * STEP) * 16)));
    };
    // B prefetch distance in k steps: kPF1 for 32-row blocks as in gemm_cols_whole, the caller's
    // for 64-row blocks as in gemm_cols_step
    constexpr int PF = RT == 1 ? kPF1 : PFB;
    f16x8 bq0[PF + 1][2], bq1[PF + 1][2];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int qd = d < nq ? d : nq - 1;
            bq0[d][p] = ldB(o0, p, qd);
            bq1[d][p] = ldB(o1, p, qd);
        }
    // the lane's row words (row rt * 32 + l32; word q / 2 covers k steps q, q + 1) and the A
    // fragment of step q: byte 2 (q & 1) + h of word q / 2
    const uint32_t* wrow = bw + l32 * WS;
    uint32_t w[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) w[rt] = wrow[rt * 32 * WS];
    auto frag = [&](int q, int rt) {
        const uint32_t byte = (w[rt] >> (16 * (q & 1) + 8 * h)) & 0xFFu;
        // (fragments built by VALU from the byte instead: neutral, r06r)
        return __builtin_bit_cast(f16x8, tab[byte]);
    };
    f16x8 af[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) af[rt] = frag(0, rt);
    const bool favored = (blockIdx.x / kCUs) & 1;  // gemm_cols' co-resident balance
    if (favored) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int q = 0; q < nq; ++q) {
        // step q + 1's operands first in program order (in flight under step q's MFMAs)
        const int qb = q + PF;
        if (qb < nq) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                bq0[qb % (PF + 1)][p] = ldB(o0, p, qb);
                bq1[qb % (PF + 1)][p] = ldB(o1, p, qb);
            }
        }
        f16x8 an[RT];
        if (q + 1 < nq) {
            if ((q & 1) == 1) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) w[rt] = wrow[rt * 32 * WS + ((q + 1) >> 1)];
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) an[rt] = frag(q + 1, rt);
        }
        if (wc.has0) {  // wave-uniform
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f16x8(&b0)[2] = bq0[q % (PF + 1)];
                acc[rt][0] = mfma_h(af[rt], b0[1], acc[rt][0]);
                acc[rt][0] = mfma_h(af[rt], b0[0], acc[rt][0]);
                if (NT >= 8 || wc.has1) {
                    const f16x8(&b1)[2] = bq1[q % (PF + 1)];
                    acc[rt][1] = mfma_h(af[rt], b1[1], acc[rt][1]);
                    acc[rt][1] = mfma_h(af[rt], b1[0], acc[rt][1]);
                }
            }
        }
        if (q + 1 < nq) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) af[rt] = an[rt];
        }
        // a scheduling fence per k step: without a barrier in the loop the scheduler would sink
        // the prefetched loads down to their uses (a full L2 / LDS round trip exposed per step)
        __builtin_amdgcn_sched_barrier(0);
    }
    if (favored) __builtin_amdgcn_s_setprio(0);
    // unscale 2^-e_n (exact), then dL/dq of the element's row, in place one group of 4 rows at
    // a time (fenced: hoisting every g load and keeping the unscaled copies beside the
    // accumulators pushed the row kernels past 256 registers, one workgroup per CU)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float4 g = *reinterpret_cast<const float4*>(gq + rt * 32 + 8 * m + 4 * h);
            const float gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = 4 * m + u;
                acc[rt][0][i] = ldexpf(acc[rt][0][i], -eb0) * gv[u];
                acc[rt][1][i] = ldexpf(acc[rt][1][i], -eb1) * gv[u];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
}

// the fp16 B images of hidden layer L (1 .. n_hidden-1): forward (B[k][n] = W_L[n][k]) and
// backward (B[k][n] = W_L[k][n]; for d_out = 1 the top layer's is Wo[k] W_L[k][n], gemm_bits)
NAV_DEV const float* img_fwd(const MlpDev& net, int L) {
    return net.packed + (int64_t)(L - 1) * 2 * split_image_floats(net.hp);
}
NAV_DEV const float* img_bwd(const MlpDev& net, int L) {
    return net.packed + (int64_t)(L - 1) * 2 * split_image_floats(net.hp) + split_image_floats(net.hp);
}

enum { IN_F32 = 0, IN_BASELINE = 1 };
enum { OUT_F32 = 0, OUT_TARGET = 1, OUT_ACT = 2, OUT_LOSS = 3, OUT_TICK = 4, OUT_TICK_POP = 5 };

// One member of a population (nav_act_tick_pop / nav_test_rollout_pop): its actor, its constants
// and its replay ring. The device-resident table [n_members] is written once per population
// (nav_pop_table_build); a workgroup's rows all belong to one member, so its entry is read
// through a block-uniform pointer.
struct PopMember {
    MlpDev net;
    nav_params p;
    float4* rows;      // the member's ring (null in a table built without rings: test rollouts)
    int64_t base_off;  // (-m * envs_per_member) mod capacity: (replay_base + base_off) % capacity
                       // + global env index is the member-local slot, so push_row's and the demo
                       // pass's (base + e) % cap hold as they are
};

struct FwdArgs {
    MlpDev net[2];
    int64_t M;
    const float* in;
    int ld_in, in_col;
    float* out[2];
    int ld_out, out_col;
    float* acts[2];
    uint32_t save_mask;  // bit L: hidden layer L's output rows are copied to acts + L*M*hp
    uint16_t* masks[2];
    // OUT_LOSS: train_critic's online twin forward with the TD error and the output layer's
    // gradient partials (robot.py:341-361)
    const float* batch;  // [M][8] replay rows (r at 4, done at 7)
    const float* qt[2];  // target twin values q1', q2' [M]
    float gamma, norm;   // discount, 2/B (mse_loss backward)
    float* dq[2];        // [M] dL/dq
    float* loss_part[2]; // [blocks] sum of (q - y)^2 over the block's rows
    float* eslab[2];     // [blocks][edge_count]: Wo / bo partials (nullable)
    int64_t ecount;
    // OUT_TARGET
    const float* eps;
    float policy_noise, noise_clip, max_action;
    uint32_t seed_lo, seed_hi, counter;
    // IN_BASELINE / OUT_ACT
    const double* state;
    const double* goal;
    const double* noise_scale;
    const double* noise_z;
    uint32_t step;
    int act_mode;
    double max_action_d;
    double* action_out;
    // OUT_TICK: the training tick of every row's env with the action just formed (one launch:
    // nav_act + nav_agent_step(_indexed); nav_act_tick)
    nav_params p;
    nav_env_soa env;
    const float2* field;
    float4* rows;
    int64_t cap, base;
    nav_step_out sout;
    DemoIdx demo;
    double* reward_out;
    // OUT_TICK_POP: the member table and the workgroups per member (net[0], rows and
    // max_action_d above are then unused and p carries the members' common seed only; cap is
    // the members' common capacity, base the common replay_base % cap)
    const PopMember* pop;
    int32_t pop_blocks;
};

// Output-layer partial sums: [d_out <= 2][4 waves][TM rows] (red_floats per block).
__host__ __device__ constexpr int red_floats(int tm) { return 2 * kWaves * tm; }

// fp16 of gemm_cols_step's split stage for TM rows: [2 planes][TM][16], then the kWaves amax
// slots. A 32-row block keeps a region of the same size (two 32-row buffers, from the per-step
// form it once ran) ahead of its slots and never touches it: moving the slots would change every
// 32-row kernel's LDS immediates
__host__ __device__ constexpr size_t stage_halves(int tm) {
    return (size_t)(tm == 32 ? 2 : 1) * 2 * tm * 16;
}
// 32-row blocks also take the whole-layer stage past the slots (gemm_cols_whole): [hp / 16 k
// steps][2 planes][32][16] fp16, hp * 128 bytes
__host__ __device__ constexpr size_t stage_bytes(int tm, int hp) {
    return stage_halves(tm) * 2 + 4 * kWaves * (tm / 32) +
           (tm == 32 ? (size_t)hp * 128 : 0);
}
template <int TM>
NAV_DEV float* amax_slots(_Float16* stage) {
    return reinterpret_cast<float*>(stage + stage_halves(TM));
}
NAV_DEV _Float16* whole_stage(_Float16* stage) {
    return stage + stage_halves(32) + 2 * kWaves;  // past the 32-row block's 4 slots (16 B)
}

// rows [tm][hp+4] + input/dy staging [tm][4] + output-layer partial sums, then the split stage
__host__ __device__ constexpr size_t lds_floats(int hp, int tm) {
    return (size_t)tm * (hp + 4) + tm * 4 + red_floats(tm);
}
inline size_t lds_bytes(int hp, int tm) { return lds_floats(hp, tm) * 4 + stage_bytes(tm, hp); }
// host: the launch sizes of what the td3_*_rows_body.inc kernels carve up. critic_rows keeps,
// between the partial sums and the stage, the sampled rows [tm][8], q1' [tm] and the row
// backward's dL/dq rows [tm][4]; actor_rows the two dy row sets [tm][4] each; its BC forms, past
// the stage, the rows' actions [2][tm] and the waves' BC sums
constexpr size_t critic_rows_lds(int tm, int hp) {
    return (lds_floats(hp, tm) + tm * 8 + tm + tm * 4) * 4 + stage_bytes(tm, hp);
}
constexpr size_t actor_rows_lds(int tm, int hp) {
    return (lds_floats(hp, tm) + tm * 8) * 4 + stage_bytes(tm, hp);
}
constexpr size_t actor_rows_bc_lds(int tm, int hp) {
    return actor_rows_lds(tm, hp) + (2 * tm + kBlock / 64) * 4;
}
// the Q-filtered BC form: past those, the rows' Q1(s, a_demo) [tm], later their keep flags
constexpr size_t actor_rows_bcq_lds(int tm, int hp) {
    return actor_rows_bc_lds(tm, hp) + tm * 4;
}


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
struct TestArgs {
    MlpDev net;              // the actor (2 -> 2)
    int64_t n;
    const double2* goal;     // env->goal
    const double4* region;   // env->region (read only when start is null)
    const double2* start;    // nullable [n]
    const float2* field;
    double max_action, goal_threshold;
    uint32_t seed_lo, seed_hi, episode;
    int32_t max_steps;
    nav_test_out out;
    // k_test_rollout<.., POP>: the member table and the workgroups per member (net, max_action and
    // goal_threshold above are then unused)
    const PopMember* pop;
    int32_t pop_blocks;
};

// bytes of the row kernels' LDS layout (lds_bytes) on the device side: the test rollout parks its
// two loop flags right behind it
__host__ __device__ constexpr size_t lds_bytes_c(int hp, int tm) {
    return lds_floats(hp, tm) * 4 + stage_bytes(tm, hp);
}

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
struct BwdArgs {
    MlpDev net[2];           // 1 or 2 networks (blockIdx.y), same shapes, same input rows
    int64_t M;
    const float* dy[2];
    int ld_dy;               // dy row stride (0: one row broadcast to every row)
    const uint16_t* masks[2];
    const float* in;         // the forward's input rows (dW0 partials), with eslab
    int ld_in, in_col;
    const float* h_top[2];   // nullable: [M][hp] top activations -> Wo / bo partials here
    float* dz[2];            // [n_hidden][M][hp], layers with a save_mask bit written
    uint32_t save_mask;
    float* dx[2];
    float* eslab[2];         // nullable: [blocks][edge_count] W0 / bias (/ Wo / bo) partials
    int64_t ecount;
};

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

// ---------------- fused TD3 row programs ----------------
// Everything in train_critic / train_actor that is local to a batch row runs as one launch per
// row block, the rows staying in LDS between the network passes (the launches that remain are
// the cross-row reductions: weight gradients and their reduce + Adam).

// ReplayBuffer.sample (robot.py:98-115) of row b: injected index or Philox with replacement
NAV_DEV void sample_row(const float* rows, int64_t size, const int64_t* idx, uint32_t s0,
                        uint32_t s1, uint32_t ctr, int64_t b, float4& lo, float4& hi) {
    int64_t k;
    if (idx) {
        k = idx[b];
    } else {
        const uint4 w = philox((uint32_t)b, 0u, NAV_TAG_SAMPLE, ctr, s0, s1);
        k = (int64_t)(((uint64_t)w.x * (uint64_t)size) >> 32);
    }
    const float4* src = reinterpret_cast<const float4*>(rows) + 2 * k;
    lo = src[0];
    hi = src[1];
}

// ---- L2 warmers for small grids ----
// A 32-row workgroup streams every weight image it multiplies by (hp^2 + hp floats per layer)
// and, alone on its XCD at small batches, each k step's B fragments arrive from beyond its L2 at
// one CU's fetch rate (~75 GB/s: ~500 cycles per step of 6 MFMAs at hp = 224, flat in the
// prefetch depth; profiles/r06za). The row kernels therefore launch, when the compute grid leaves
// most CUs idle, extra workgroup rows (blockIdx.y >= y0) that only touch one 4-B word per 128-B
// line of the launch's images, in the order the compute workgroups consume them, so the lines
// are in each XCD's L2 before the compute workgroups ask. Blocks are dealt round-robin over the
// 8 XCDs (MI355X_MICROARCH: b and b + 8 share one; speed only, never correctness): the warmers
// with equal (index mod 8) split the image list between them.
constexpr int kWarmMax = 16;         // image ranges per launch
constexpr int kWarmPerXcd = 16;      // warmer workgroups per XCD
constexpr int64_t kWarmGrid = 128;   // compute workgroups up to which warmers are launched
struct WarmList {
    int y0;                          // grid rows of compute workgroups (warmers: rows >= y0)
    int n;                           // ranges (0: no warmers)
    const char* p[kWarmMax];
    uint32_t bytes[kWarmMax];
};

NAV_DEV void warm_l2(const WarmList& w) {
    const uint32_t j = blockIdx.x + gridDim.x * (blockIdx.y - (uint32_t)w.y0);
    const uint32_t nw = gridDim.x * (gridDim.y - (uint32_t)w.y0);
    const uint32_t cnt = (nw - (j & 7u) + 7u) >> 3, rank = j >> 3;  // warmers of this XCD
    uint32_t x = 0;
    for (int i = 0; i < w.n; ++i) {
        const uint32_t lines = (w.bytes[i] + 127u) >> 7;
        const uint32_t per = (lines + cnt - 1u) / cnt;
        const uint32_t l1 = min(lines, (rank + 1u) * per);
        const char* p = w.p[i];
#pragma unroll 4
        for (uint32_t l = rank * per + threadIdx.x; l < l1; l += kBlock)
            x ^= *reinterpret_cast<const uint32_t*>(p + ((size_t)l << 7));
    }
    asm volatile("" ::"v"(x));  // keeps the loads
}

// host: append [p, p + bytes) to the list; false when full
inline bool warm_add(WarmList& w, const float* p, int64_t floats) {
    if (w.n >= kWarmMax) return false;
    w.p[w.n] = reinterpret_cast<const char*>(p);
    w.bytes[w.n++] = (uint32_t)(floats * 4);
    return true;
}
// host: a network's forward images (layers 1 .. nh-1), or its whole packed buffer (all images)
inline bool warm_net(WarmList& w, const MlpDev& net, bool fwd_only) {
    if (net.n_hidden < 2) return true;
    const int64_t im = split_image_floats(net.hp);
    if (!fwd_only) return warm_add(w, net.packed, (int64_t)(net.n_hidden - 1) * 2 * im);
    for (int L = 1; L < net.n_hidden; ++L)
        if (!warm_add(w, net.packed + (int64_t)(L - 1) * 2 * im, im)) return false;
    return true;
}
// host: grid rows of warmers for a compute grid of gx x gy (0: none)
inline unsigned warm_rows(const WarmList& w, unsigned gx, unsigned gy) {
    if (w.n == 0 || (int64_t)gx * gy > kWarmGrid) return 0;
    return (8u * kWarmPerXcd + gx - 1) / gx;
}

struct CriticRowsArgs {
    MlpDev actor_t, critic_t[2], critic[2];
    int64_t B;
    const float* rows;
    int64_t rsize;
    const int64_t* idx;
    uint32_t seed_lo, seed_hi, sample_ctr, noise_ctr;
    const float* eps;
    float policy_noise, noise_clip, max_action, gamma, norm;
    float* batch;
    float* dq[2];
    float* loss_part[2];
    float* eslab[2];
    int64_t ecount;
    float* acts[2];
    uint32_t save_mask;
    uint16_t* masks[2];
    int row_backward;     // also each online critic's row backward (robot.py:361 .backward())
    int split_twins;      // grid.y = 2: workgroup y runs online critic y only (small batches)
    float* dz[2];         // [nh][B][hp] dz rows of dz_save_mask layers (row_backward)
    uint32_t dz_save_mask;
    WarmList warm;        // set by the launcher
};
static_assert(sizeof(CriticRowsArgs) <= 4096, "kernel argument size");

// The population forms of critic_rows / actor_rows (nav_td3_critic_rows_pop / _actor_rows_pop):
// grid.z is the member, whose CriticRowsArgs / ActorRowsArgs the workgroup reads from the device
// table (nav_td3_pop_table_build) through a block-uniform pointer. What changes per launch and is
// common to all members travels by value, so the table is not rewritten while training: the
// replay fill, the Philox counter, and the twins' form (chosen from all members' workgroups).
struct RowsPop {
    const void* table;  // [n_members] CriticRowsArgs or ActorRowsArgs
    int64_t size;
    uint32_t counter;
    int32_t split_twins;
};

// train_critic (robot.py:329-361) for one block of TM batch rows: sample, target policy
// smoothing through the target actor, twin target critics, TD target, then the twin online
// critics with mse_loss's gradient, the loss and the output layers' gradient partials, and
// (row_backward) each online critic's row backward with its W0 / bias partials right after its
// forward, while its rows and ReLU bits are fresh.
// CBM: the critics' row-backward form (bwd_net's BM: 0 for one hidden layer, else 1), chosen by
// the launcher from n_hidden
// The kernel's statements are td3_critic_rows_body.inc, once per form: the plain kernel's stay
// token for token what they were (its machine code is pinned, tools/isa_diff.py), the population
// form (POP) reads `a` from the member's table entry and the launch's values from `pv` (the
// entry's rsize, counters, split_twins and warm list are then unused).
// The weighted form (nav_td3_critic_rows_w, prioritised replay): the plain arguments and, beside
// them, the rows' importance weights and the |TD error| outputs. Not in CriticRowsArgs: the
// population table stores that struct per member.
struct CriticPerExtra {
    const float* w;      // [B] importance weights
    float* td_abs[2];    // [B] |q_i - y| per online critic
};
struct CriticRowsWArgs {
    CriticRowsArgs r;
    CriticPerExtra per;
};
static_assert(sizeof(CriticRowsWArgs) <= 4096, "kernel argument size");

template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows(CriticRowsArgs a) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr bool WEIGHTED = false;
    constexpr CriticPerExtra px{};
#include "td3_critic_rows_body.inc"
}
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr bool WEIGHTED = false;
    constexpr CriticPerExtra px{};
    const CriticRowsArgs& a = static_cast<const CriticRowsArgs*>(pv.table)[blockIdx.z];
#include "td3_critic_rows_body.inc"
}
// the weighted form (WEIGHTED: loss_epilogue scales dq and the loss term by px.w and writes
// px.td_abs; everything downstream reads the weighted dq)
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_critic_rows_w(CriticRowsWArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr bool WEIGHTED = true;
    const CriticRowsArgs& a = x.r;
    const CriticPerExtra& px = x.per;
#include "td3_critic_rows_body.inc"
}

struct ActorRowsArgs {
    MlpDev actor, critic;
    int64_t B;
    const float* rows;
    int64_t rsize;
    const int64_t* idx;
    uint32_t seed_lo, seed_hi, sample_ctr;
    float dq;            // d(-mean Q)/dQ = -1/B
    float* batch;        // [B][8] sampled rows
    float* q;            // [B] Q1(s, pi(s)), nullable
    float* da;           // [B][2] dL/da
    float* acts;         // actor [nh][B][hp], save_mask layers (the top one feeds dWo)
    uint32_t save_mask;
    float* dz;           // actor [nh][B][hp], dz_save_mask layers
    uint32_t dz_save_mask;
    uint16_t* masks_a;
    uint16_t* masks_c;
    float* eslab;        // actor edge partials
    int64_t ecount;
    WarmList warm;       // set by the launcher
};

// The behaviour-cloning forms of actor_rows (nav_td3_actor_rows_bc): the plain arguments (dq =
// -q_weight/B) and, beside them, what the BC term on the batch's first B_demo rows needs. Not in
// ActorRowsArgs: the population table stores that struct per member.
enum { ACTOR_PLAIN = 0, ACTOR_TD3_BC = 1, ACTOR_BC_ONLY = 2, ACTOR_TD3_BCQ = 3 };
struct ActorBcExtra {
    int64_t B_demo;      // rows b < B_demo are demonstration rows
    float bc_coef;       // 2 * bc_weight / B_demo
    float* bc_part;      // [row blocks] block sums of (pi_j - a_j)^2 over demonstration rows
};
struct ActorRowsBcArgs {
    ActorRowsArgs r;     // r.critic: the actor's descriptor again when bc_only (never read)
    ActorBcExtra bc;
    int bc_only;         // no critic given: the BC term alone
};
// The Q-filtered BC form (nav_td3_actor_rows_bcq, MODE = ACTOR_TD3_BCQ): a demonstration row b <
// B_demo adds its BC term only where keep_b = Q1(s_b, a_b) > Q1(s_b, pi(s_b)) (online critic 1,
// strict; a NaN on either side compares false: dropped). The decision carries no gradient, and
// the term's normaliser stays B_demo, not the kept rows' count: bc_coef stays a launch constant
// and no count crosses the blocks before the backward pass. Not in ActorBcExtra: the
// population's BC table stores ActorRowsBcArgs per member.
struct ActorBcqExtra {
    float* q_demo;       // [B] Q1(s, a_demo), rows < B_demo written; nullable
    int32_t* keep_part;  // [row blocks] demonstration rows of the block the filter kept
};
struct ActorRowsBcqArgs {
    ActorRowsBcArgs b;   // bc_only 0: the filter needs the critic
    ActorBcqExtra qf;
};

// train_actor (robot.py:382-390) for one block of TM batch rows: sample, actor forward,
// critic-1 forward on (s, pi(s)), backward of -mean(Q) through critic 1 to its action input
// (critic grads discarded, as zero_grad does), and the actor's row backward with its edge
// partials.
// (td3_actor_rows_body.inc once per form, as k_td3_critic_rows)
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows(ActorRowsArgs a) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr int MODE = ACTOR_PLAIN;
    constexpr ActorBcExtra bx{};
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr int MODE = ACTOR_PLAIN;
    constexpr ActorBcExtra bx{};
    constexpr ActorBcqExtra qx{};
    const ActorRowsArgs& a = static_cast<const ActorRowsArgs*>(pv.table)[blockIdx.z];
#include "td3_actor_rows_body.inc"
}
// the BC forms (MODE = ACTOR_TD3_BC / ACTOR_BC_ONLY; the latter runs no critic pass, so its CBM
// is unused and the launcher takes 1)
template <int NT, int RT, int CBM, int MODE>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bc(ActorRowsBcArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    const ActorRowsArgs& a = x.r;
    const ActorBcExtra& bx = x.bc;
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}
// the Q-filtered BC form: in the workgroups that hold demonstration rows (row0 < B_demo, the
// batch's prefix) one more forward of the critic, on (s, a_demo), ahead of the actor's
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bcq(ActorRowsBcqArgs x) {
    constexpr bool POP = false;
    constexpr RowsPop pv{};
    constexpr int MODE = ACTOR_TD3_BCQ;
    const ActorRowsArgs& a = x.b.r;
    const ActorBcExtra& bx = x.b.bc;
    const ActorBcqExtra& qx = x.qf;
#include "td3_actor_rows_body.inc"
}
// the population's BC form (nav_td3_actor_rows_bc_pop): grid.z is the member, whose
// ActorRowsBcArgs the workgroup reads from the BC table (nav_td3_pop_bc_table_build) through a
// block-uniform pointer; size and counter from `pv` as in k_td3_actor_rows_pop
template <int NT, int RT, int CBM>
__global__ __launch_bounds__(kBlock, 1) void k_td3_actor_rows_bc_pop(RowsPop pv) {
    constexpr bool POP = true;
    constexpr int MODE = ACTOR_TD3_BC;
    const ActorRowsBcArgs& x = static_cast<const ActorRowsBcArgs*>(pv.table)[blockIdx.z];
    const ActorRowsArgs& a = x.r;
    const ActorBcExtra& bx = x.bc;
    constexpr ActorBcqExtra qx{};
#include "td3_actor_rows_body.inc"
}

// what a population launch passes to the per-NT objects (the table's row sections are
// [n_members] CriticRowsArgs, then [n_members] ActorRowsArgs; the BC table's is [n_members]
// ActorRowsBcArgs)
struct RowsPopLaunch {
    RowsPop k;
    int64_t B;
    int n_hidden, n_members;
};


// ---- launch helpers (template dispatch on NT = hp / 32 and RT = rows / 32) ----
// Workgroup height: RT = 2 (64 rows, two workgroups per CU so one workgroup's epilogue overlaps
// the other's MFMA loop; RT = 4, 128 rows and one workgroup per CU, measured slower in round 1:
// profiles/r01c_micro_rt4.json, no longer built).
// Small batches take RT = 1 (32-row workgroups): at M <= kSmallRows the 64-row grid leaves CUs
// idle (config 1's 100 rows: 2 workgroups), and a 32-row block halves each wave's MFMA chain per
// layer, so the latency-bound small-batch learner runs twice the workgroups at half the chain.
// Not for the fused tick (its demo pass works on whole waves of envs).
constexpr int64_t kSmallRows = 16384;
int row_tiles_for(int64_t M, bool tick) { return (!tick && M <= kSmallRows) ? 1 : 2; }

// The row kernels (forward, row backward, critic_rows, actor_rows) are instantiated per NT in
// their own objects (mlp_rows_nt.hip built with NAV_MLP_PART = NT, see the Makefile) so the heavy
// template instantiations compile in parallel; the C ABI's object (mlp_abi.hip) dispatches to
// them through nav_mlp_rows_<role>_<NT>(). Argument structs travel as const void* (same definitions).
enum {
    FAM_FWD = 0, FAM_BWD = 1, FAM_CRITIC = 2, FAM_ACTOR = 3, FAM_TEST = 4, FAM_TEST_POP = 5,
    FAM_CRITIC_POP = 6, FAM_ACTOR_POP = 7, FAM_ACTOR_BC = 8, FAM_ACTOR_BC_POP = 9, FAM_CRITIC_W = 10,
    FAM_ACTOR_BCQ = 11
};

}  // namespace
