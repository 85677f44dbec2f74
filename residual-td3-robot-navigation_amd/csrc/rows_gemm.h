// rows_gemm.h — the hidden x hidden products of the row kernels on gfx950: one 256-thread
// workgroup = 4 waves = a block of 64 rows (32 for small batches) kept in LDS as fp32 (row stride
// hp+4) across all layers. Hidden x hidden layers run on the fp16 matrix cores
// (v_mfma_f32_32x32x16_f16) at f32-class accuracy: each fp32 operand is scaled by a power of two
// (A per 32-row tile, B per column) and split into two fp16 planes (hi + lo carries 22
// significant bits), and the three products lo.hi + hi.lo + hi.hi accumulate in fp32
// (mlp_common.h; tests/test_gpu_mlp.py pins the result against an fp64 reference at 2e-6 of
// scale). Every wave owns 1-2 32-column tiles of all the block's rows; the A operand is split
// once per k step into an LDS stage shared by the 4 waves, the B operand streams from the
// L2-resident split weight image (refreshed after Adam / Polyak). Here: the wave's column tiles,
// the A-scale slots and stages (their sizes are rows_args.h's), gemm_cols in its two forms, the
// bit-operand product gemm_bits of the row backward's top layer, and the weight images of a layer.
#pragma once
#include "rows_args.h"


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
NAV_DEV float* amax_slots(_Float16* stage) {
    return reinterpret_cast<float*>(stage + stage_halves(TM));
}
NAV_DEV _Float16* whole_stage(_Float16* stage) {
    return stage + stage_halves(32) + 2 * kWaves;  // past the 32-row block's 4 slots (16 B)
}

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

}  // namespace
