// wgrad.h — the device code of the hidden x hidden weight gradients on MFMA: the argument struct,
// the tilings and the tile bodies that the plain kernels (learner_kernels.hip) and the population
// kernels (learner_pop.hip) wrap. Nothing host-side here but sizes and the tiling.
#pragma once
#include "mlp_common.h"

namespace {

// ---------------- hidden x hidden weight gradients (split-M partial slabs) ----------------
// dW_L = dz_L^T h_{L-1} for L = 1 .. nh-1 over the rows of each split. The thin layers' gradients
// (W0, every bias, Wo, bo) are edge partials of the forward / backward kernels instead.
//
// Work decomposition: one workgroup = 8 waves = one tn x 64 output tile (n0.., k0..) of one
// layer of one network over the rows of one split; each wave takes 1/8 of the split's rows and
// keeps the tile in 32 x 32 accumulators (the MFMA K dimension is the batch row), the 8 partial
// tiles are summed through LDS in a fixed order and the workgroup writes ONE partial slab tile.
// 256 workgroups (one per CU, 2 waves per SIMD) fill the chip, so the slabs are 4-8 MB per
// launch and the reduce reads 8-16 slabs.
// 2-hidden-layer networks with whole tiles (the bench shape) take the factored path
// (wgrad_rows_fact: the ReLU bit as an exact bf16 A operand, Wo applied after the sum; for
// d_out = 1 the tile is 256 x 32 at hp 256 and 128 x 64 at hp 128). Every other shape takes the
// f32 MFMA path below (tn = 64).
// Operands come straight from registers, no panel staging and no barrier in the row loop: for
// the batch rows (2 per MFMA step: lane half h = row parity) every lane forms its own A element
// P[row][n0 + 32 i + lane] and B element Q[row][k0 + 32 j + lane]. P = dz of the top hidden
// layer is recomputed as top_unit(dy row, Wo column) under the forward's ReLU bit; Q = h_0 as
// layer0_unit(x row, W0 row, b0) — the same bits the backward / forward produced, so a 2-hidden-
// layer network reads only its input rows, dy rows and 1 bit per element. The row data (x, dy)
// of 64 rows is loaded coalesced (lane = row), parked in a wave-private LDS slot and read back
// as a broadcast per lane half; saved panels of deeper networks are read per element.
struct WgradArgs {
    MlpDev net[2];          // 1 or 2 networks, same shapes, same input rows
    int64_t M;
    const float* in;        // layer-0 input rows: h_0 is recomputed (layer0_unit)
    int ld_in, in_col;
    const float* acts[2];   // [nh][M][hp]: saved h_L, 1 <= L <= nh-2
    const float* dz[2];     // [nh][M][hp]: saved dz_L, 1 <= L <= nh-2
    const float* dy[2];     // dz_{nh-1} is recomputed: top_unit(dy row, Wo) under the ReLU bit
    int ld_dy;
    const uint16_t* masks[2];  // the forward's ReLU bit image
    float* slabs[2];        // [splits][(nh-1) hp hp]
    int splits;
    int tk;                 // tile width on the k side: 64, or 32 (the 256 x 32 factored form)
    int TT;                 // tk-wide tiles across hp (the k side of a tile)
    int tn;                 // tile height on the n side: 64, or 128 / 256 (wgrad_tile_fact)
    int TN;                 // tn-high tiles across hp
    int n_hid;              // tile jobs per network = (nh - 1) * TN * TT
    int fact;               // 1: the factored-Wo path (wgrad_tile_fact) for every tile
    int64_t per_split;      // rows per split (multiple of 32)
    int64_t per_wave;       // rows per wave (multiple of 32)
    int64_t skew;           // rows moved from each of waves 4-7 to its SIMD partner wave w - 4
};

// Phase probe of the weight-gradient kernels (variant builds with -DNAV_WGRAD_TRACE only;
// tools/wgrad_trace.py): s_memtime per wave at numbered marks of 4 workgroups (blocks 0, 1, 128,
// 255) per kernel (0 k_wgrad_fact, 1 k_wgrad); the last launch of each kernel wins.
#ifdef NAV_WGRAD_TRACE
__device__ unsigned long long g_wgrad_trace[2][4][8][8];
#define WG_MARK(kid, k)                                                                        \
    do {                                                                                       \
        const int b_ = blockIdx.x == 0 ? 0 : blockIdx.x == 1 ? 1 : blockIdx.x == 128 ? 2         \
                       : blockIdx.x == 255 ? 3 : -1;                                           \
        if (b_ >= 0 && (threadIdx.x & 63) == 0)                                                \
            g_wgrad_trace[kid][b_][threadIdx.x >> 6][k] = __builtin_readcyclecounter();         \
    } while (0)
#else
#define WG_MARK(kid, k) \
    do {                \
    } while (0)
#endif

constexpr int WG_WAVES = 8;
#ifndef NAV_WG_SKEW_FACT
#define NAV_WG_SKEW_FACT 64
#endif
#ifndef NAV_WG_SKEW_OPND
#define NAV_WG_SKEW_OPND 128
#endif
constexpr int WG_TOTAL = 256;  // workgroups that fill the chip (one 8-wave workgroup per CU)
constexpr int WG_THREADS = WG_WAVES * 64;
constexpr int WG_TILE = 64;
constexpr int WG_CHUNK = 64;  // rows per staged chunk (lane = row)
// LDS: 8 partial 64 x 64 tiles for the in-workgroup reduction + per wave 64 rows of (x[4], dy[2])
constexpr int WG_STAGE_FLOATS = WG_CHUNK * 6;  // one slot; 2 slots per wave (double buffer)
inline size_t wgrad_lds_bytes() {
    return ((size_t)WG_WAVES * WG_TILE * WG_TILE + (size_t)WG_WAVES * 2 * WG_STAGE_FLOATS) * 4;
}
// The factored path's tile: for d_out = 1 a wave holds 128 accumulator registers, as 256 (n) x 32
// (k) when hp % 256 == 0 (NI = 8 column tiles of n, one 32-column half of k: every B operand
// Q = g relu(h_0) is formed once per launch, where two 128 x 64 tiles with the same k0 formed it
// twice), as 128 x 64 (NI = 4, two halves) when hp % 128 == 0, else 64 x 64. The path itself needs
// a 2-hidden-layer network with whole 64 x 64 tiles.
__host__ __device__ inline bool wgrad_fact_ok(int hp, int n_hidden) {
    return n_hidden == 2 && hp % WG_TILE == 0;
}
// the tile shape and the tile jobs per network of a launch: the one source for the grid
// (nav_mlp_wgrad), the split count (nav_mlp_wgrad_splits) and the job decode (wgrad_job)
struct WgradTiling {
    int tn, tk, TN, TT, jobs;
};
inline WgradTiling wgrad_tiling(int d_out, int hp, int n_hidden) {
    WgradTiling t;
    const bool f1 = wgrad_fact_ok(hp, n_hidden) && d_out == 1;
    const bool wide = f1 && hp % 256 == 0;
    t.tn = wide ? 256 : f1 && hp % 128 == 0 ? 128 : WG_TILE;
    t.tk = wide ? 32 : WG_TILE;
    t.TN = (hp + t.tn - 1) / t.tn;
    t.TT = (hp + t.tk - 1) / t.tk;
    t.jobs = (n_hidden > 1 ? n_hidden - 1 : 0) * t.TN * t.TT;
    return t;
}

// rows [r_lo, r_hi) of one wave into acc (tile n0.., k0.. of layer L of net y)
// RA (k_wgrad_gen): the chunk's saved dz / h row values are loaded into registers before its
// products (loaded at their use inside the product they exposed one memory round trip per row
// pair: ~20 k cycles for 32 rows at config 1's shape, profiles/r06zj); k_wgrad, whose MFMA-operand
// path holds 254 registers, keeps the loads at their use
template <bool PR, bool QR, bool RA_ = false>
NAV_DEV void wgrad_rows(const WgradArgs& a, int y, int L, int n0, int k0, int64_t r_lo,
                        int64_t r_hi, float* stage, f32x16 (&acc)[2][2]) {
    const MlpDev& net = a.net[y];
    const int hp = net.hp, nh = net.n_hidden, d_in = net.d_in, d_out = net.d_out;
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int64_t M = a.M, MH = M * hp;
    // 32-column sub-tiles inside hp (wave-uniform); absent columns read a clamped valid column
    const bool nv1 = n0 + 32 < hp, kv1 = k0 + 32 < hp;
    const int cn[2] = {n0 + l32, nv1 ? n0 + 32 + l32 : n0 + l32};
    const int ck[2] = {k0 + l32, kv1 ? k0 + 32 + l32 : k0 + l32};
    float wo[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, w0[2][4] = {}, b0[2] = {0.f, 0.f};
    if (PR) {
        const float* Wo = net.params + net.w_off[nh];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wo[i][0] = Wo[cn[i]];
            wo[i][1] = d_out > 1 ? Wo[hp + cn[i]] : 0.f;
        }
    }
    if (QR) {
        const float* W0 = net.params + net.w_off[0];
        const float* bb = net.params + net.b_off[0];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) w0[j][k] = k < d_in ? W0[ck[j] * d_in + k] : 0.f;
            b0[j] = bb[ck[j]];
        }
    }
    // one saved operand only (two would not fit next to the accumulators), HS row pairs at a time
    constexpr bool RA = RA_ && (PR != QR);
    constexpr int HS = WG_CHUNK / 8;  // row pairs per register window
    const int NTm = hp >> 5;
    const uint16_t* mk = PR ? a.masks[y] + (size_t)(nh - 1) * mask_rowtiles(M) * NTm * 64 : nullptr;
    const int tm0 = n0 >> 5, tm1 = nv1 ? tm0 + 1 : tm0;
    const float* Psv = PR ? nullptr : a.dz[y] + (int64_t)L * MH;
    const float* Qsv = QR ? nullptr : a.acts[y] + (int64_t)(L - 1) * MH;
    float* xs = stage;                  // [64][4]
    float* gs = stage + WG_CHUNK * 4;   // [64][2]

    // one chunk's row data in registers: x row (QR), dy row (PR), and the ReLU words of the
    // chunk's 2 row tiles x 2 column tiles (PR): bits of rows with (row & 4) == 0 in the low half
    float4 cx = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 cg = make_float2(0.f, 0.f);
    uint32_t cm[2][2] = {{0u, 0u}, {0u, 0u}};
    auto load = [&](int64_t rb) {
        const int64_t r = rb + lane;
        const bool ok = r < r_hi;
        const int64_t rc = ok ? r : r_lo;
        if (QR) {
            const float* x = a.in + rc * a.ld_in + a.in_col;
            cx.x = ok ? x[0] : 0.f;
            cx.y = ok && d_in > 1 ? x[1] : 0.f;
            cx.z = ok && d_in > 2 ? x[2] : 0.f;
            cx.w = ok && d_in > 3 ? x[3] : 0.f;
        }
        if (PR) {
            const float* g = a.dy[y] + rc * a.ld_dy;
            cg.x = ok ? g[0] : 0.f;
            cg.y = ok && d_out > 1 ? g[1] : 0.f;
            const int64_t rt0 = rb >> 5;
            const bool t1 = rb + 32 < r_hi;  // a range may end after the chunk's first tile
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const uint16_t* w = mk + ((rt0 + (t && t1)) * NTm + (i ? tm1 : tm0)) * 64 + l32;
                    cm[i][t] = t && !t1 ? 0u : (uint32_t)w[0] | ((uint32_t)w[32] << 16);
                }
        }
    };
    auto park = [&]() {
        if (QR) *reinterpret_cast<float4*>(xs + lane * 4) = cx;
        if (PR) *reinterpret_cast<float2*>(gs + lane * 2) = cg;
    };
    if (r_lo >= r_hi) return;
    load(r_lo);
    park();
    uint32_t mw[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) mw[i][t] = cm[i][t] >> h;  // the lane half's row parity
    for (int64_t rb = r_lo; rb < r_hi; rb += WG_CHUNK) {
        const bool more = rb + WG_CHUNK < r_hi;
        if (more) load(rb + WG_CHUNK);  // next chunk in flight under this one
        float ps[RA && !PR ? HS : 1][2], qs[RA && !QR ? HS : 1][2];
        auto window = [&](int s0) {  // the saved row values of row pairs s0 .. s0 + HS - 1
#pragma unroll
            for (int u = 0; u < HS; ++u) {
                const int64_t r = rb + 2 * (s0 + u) + h;
                const bool ok = r < r_hi;
                const int64_t rc = ok ? r : r_lo;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if constexpr (!PR) ps[u][i] = ok ? Psv[rc * hp + cn[i]] : 0.f;
                    if constexpr (!QR) qs[u][i] = ok ? Qsv[rc * hp + ck[i]] : 0.f;
                }
            }
        };
#pragma unroll
        for (int s = 0; s < WG_CHUNK / 2; ++s) {
            // wave-uniform: a range's last chunk may be short (RA stops at a window boundary: the
            // window's rows past r_hi add exact zeros, and its row registers stay static)
            if ((!RA || s % HS == 0) && rb + 2 * s >= r_hi) break;
            if constexpr (RA) {
                if (s % HS == 0) window(s);
            }
            const int rr = 2 * s + h;  // row of this lane half inside the chunk
            float p[2], q[2];
            if (PR) {
                const float2 g = *reinterpret_cast<const float2*>(gs + rr * 2);
                // bit of row rr in the C-layout mask word: element (rr & 3) + 4 (rr >> 3 & 3) of
                // lane half (rr >> 2) & 1 (the +h of rr was folded into mw)
                const int sh = 16 * ((s >> 1) & 1) + 2 * (s & 1) + 4 * ((s & 15) >> 2);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const uint32_t bit = (mw[i][s >> 4] >> sh) & 1u;
                    p[i] = bit ? top_unit(g.x, g.y, wo[i][0], wo[i][1]) : 0.f;
                }
            } else if constexpr (RA) {
#pragma unroll
                for (int i = 0; i < 2; ++i) p[i] = ps[RA && !PR ? s % HS : 0][i];
            } else {
                const int64_t r = rb + rr;
                const bool ok = r < r_hi;
                const float* src = Psv + (ok ? r : r_lo) * hp;
#pragma unroll
                for (int i = 0; i < 2; ++i) p[i] = ok ? src[cn[i]] : 0.f;
            }
            if (QR) {
                const float4 x = *reinterpret_cast<const float4*>(xs + rr * 4);
#pragma unroll
                for (int j = 0; j < 2; ++j) q[j] = layer0_unit(x, w0[j][0], w0[j][1], w0[j][2], w0[j][3], b0[j]);
            } else if constexpr (RA) {
#pragma unroll
                for (int j = 0; j < 2; ++j) q[j] = qs[RA && !QR ? s % HS : 0][j];
            } else {
                const int64_t r = rb + rr;
                const bool ok = r < r_hi;
                const float* src = Qsv + (ok ? r : r_lo) * hp;
#pragma unroll
                for (int j = 0; j < 2; ++j) q[j] = ok ? src[ck[j]] : 0.f;
            }
            acc[0][0] = mfma(p[0], q[0], acc[0][0]);
            if (kv1) acc[0][1] = mfma(p[0], q[1], acc[0][1]);
            if (nv1) acc[1][0] = mfma(p[1], q[0], acc[1][0]);
            if (nv1 && kv1) acc[1][1] = mfma(p[1], q[1], acc[1][1]);
        }
        if (more) {
            park();  // this wave's reads of the slot were issued above: LDS keeps them in order
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 2; ++t) mw[i][t] = cm[i][t] >> h;
        }
    }
}

// Wave-uniform max |dy_d| (d < d_out) and max |x_i| (i < d_in) over the wave's rows [r_lo, r_hi):
// the bounds behind the fp16 operand scales of the weight-gradient products (a bound within a
// few binades of the true max costs nothing: the lo plane's absolute step stays 2^-24 of the
// scaled bound).
NAV_DEV void row_maxima(const WgradArgs& a, int y, int64_t r_lo, int64_t r_hi, float (&G)[2],
                        float (&X)[4]) {
    const int lane = threadIdx.x & 63, d_in = a.net[y].d_in, d_out = a.net[y].d_out;
    float g0 = 0.f, g1 = 0.f, x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
    // RU rows per lane per trip, every load of a trip issued before the first max (one memory
    // round trip per 64 RU rows), whole-row vector loads where the layout allows (the rows are
    // 32 B apart in the learner's batch: one load instruction per row instead of d_in)
    constexpr int RU = 4;
    const float* xin = a.in + a.in_col;
    const bool xv4 = d_in == 4 && (a.ld_in & 3) == 0 && ((uintptr_t)xin & 15) == 0;
    const bool xv2 = d_in == 2 && (a.ld_in & 1) == 0 && ((uintptr_t)xin & 7) == 0;
    const bool gv2 = d_out == 2 && (a.ld_dy & 1) == 0 && ((uintptr_t)a.dy[y] & 7) == 0;
    for (int64_t rb = r_lo; rb < r_hi; rb += 64 * RU) {
        float gv[RU][2], xv[RU][4];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            gv[u][0] = gv[u][1] = 0.f;
            xv[u][0] = xv[u][1] = xv[u][2] = xv[u][3] = 0.f;
            if (rb + 64 * u >= r_hi) continue;  // wave-uniform
            const int64_t r = rb + 64 * u + lane;
            if (r >= r_hi) continue;
            const float* g = a.dy[y] + r * a.ld_dy;
            const float* x = xin + r * a.ld_in;
            if (gv2) {
                const float2 v = *reinterpret_cast<const float2*>(g);
                gv[u][0] = v.x;
                gv[u][1] = v.y;
            } else {
                gv[u][0] = g[0];
                if (d_out > 1) gv[u][1] = g[1];
            }
            if (xv4) {
                const float4 v = *reinterpret_cast<const float4*>(x);
                xv[u][0] = v.x; xv[u][1] = v.y; xv[u][2] = v.z; xv[u][3] = v.w;
            } else if (xv2) {
                const float2 v = *reinterpret_cast<const float2*>(x);
                xv[u][0] = v.x; xv[u][1] = v.y;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (d_in > i) xv[u][i] = x[i];
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            g0 = fmaxf(g0, fabsf(gv[u][0]));
            g1 = fmaxf(g1, fabsf(gv[u][1]));
            x0 = fmaxf(x0, fabsf(xv[u][0]));
            x1 = fmaxf(x1, fabsf(xv[u][1]));
            x2 = fmaxf(x2, fabsf(xv[u][2]));
            x3 = fmaxf(x3, fabsf(xv[u][3]));
        }
    }
    // wave-uniform: scalar registers
    auto su = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wave_max_abs(v)))); };
    G[0] = su(g0);
    G[1] = su(g1);
    X[0] = su(x0);
    X[1] = su(x1);
    X[2] = su(x2);
    X[3] = su(x3);
}

// Bound on |h_0[r][c]| = relu(b0[c] + sum_i x_ri W0[c][i]) for the column c of this lane from the
// lane half's constants (inputs h and 2 + h; the bias on h = 0): sum_i X_i |W0[c][i]| + |b0[c]|.
NAV_DEV float h0_bound(const float (&X)[4], float wa, float wb, float bias) {
    const int h = (threadIdx.x & 63) >> 5;
    const float part = (h ? X[1] : X[0]) * fabsf(wa) + (h ? X[3] : X[2]) * fabsf(wb) + fabsf(bias);
    return part + __shfl_xor(part, 32, 64);
}

// The largest exponent <= e at which a constant of magnitude <= m stays finite when scaled by
// 2^e (m 2^e < 2^126). The h_0 scale comes from the bound above, which is tiny when the inputs
// and the bias are: the layer-0 weights scaled by it would overflow to inf and a zero input row
// then give 0 * inf = NaN in the operand MFMA. Binds only in that degenerate case (the bound's
// own 2^14 target keeps e below it otherwise), so normal results are unchanged.
NAV_DEV int cap_exp_finite(int e, float m) {
    if (!(m > 0.f)) return e;
    int E;
    (void)frexpf(m, &E);  // m = f 2^E, f in [0.5, 1)
    return min(e, 126 - E);
}

// The MFMA-operand path for a full 64 x 64 tile of a 2-hidden-layer network with d_out = 2 (the
// actor; d_out = 1 takes the factored path below).
// The operands are produced by MFMAs too: per 32-row tile, dz = dy . Wo (K = d_out <= 2, one
// v_mfma_f32_32x32x2_f32 per 32 columns) and h_0 = x . W0^T + b0 (K = d_in <= 4, two MFMAs on
// the bias as C) land in the C layout, where lane (l32, h) register e holds row
// acc_row(e, h) of column l32. Taking the weight-gradient MFMA's K (batch-row) order as
// step e <-> rows {acc_row(e, 0), acc_row(e, 1)}, register e of those tiles IS the A / B operand
// of step e, and bit e of the lane's own ReLU mask word (the forward's C-layout image) is the
// ReLU derivative of exactly that element. Per 64 weight-gradient MFMAs a wave issues 6 operand
// MFMAs and ~100 VALU (mask, relu) instead of ~320 VALU: the f32 MFMA shares the SIMD's issue
// with the VALU, so the VALU count per MFMA is what sets the rate. No LDS, no barrier in the
// row loop. h_0 and dz are the forward's / backward's values as fused f32 chains in the same
// order (layer0_unit: b + x0 w0 + x1 w1 + ..., top_unit: g0 w0 + g1 w1).
NAV_DEV void wgrad_rows_mfma(const WgradArgs& a, int y, int n0, int k0, int64_t r_lo,
                             int64_t r_hi, f32x16 (&acc)[2][2]) {
    const MlpDev& net = a.net[y];
    const int hp = net.hp, nh = net.n_hidden, d_in = net.d_in, d_out = net.d_out;
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int64_t M = a.M;
    const int NTm = hp >> 5;
    // constant B operands of the operand MFMAs: Wo rows (k = output j = h), W0 columns (k = h,
    // then 2 + h), and the bias through a K = 2 MFMA of (1, 0) x (b, 0): the C tile starts at b
    // exactly, so h_0 accumulates in layer0_unit's order b + x0 w0 + x1 w1 + x2 w2 + x3 w3
    float wob[2], w0b[2][2], bob[2];
    {
        const float* Wo = net.params + net.w_off[nh];
        const float* W0 = net.params + net.w_off[0];
        const float* bb = net.params + net.b_off[0];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wob[i] = h < d_out ? Wo[h * hp + n0 + 32 * i + l32] : 0.f;
            const int c = k0 + 32 * i + l32;
            w0b[i][0] = h < d_in ? W0[c * d_in + h] : 0.f;
            w0b[i][1] = 2 + h < d_in ? W0[c * d_in + 2 + h] : 0.f;
            bob[i] = h == 0 ? bb[c] : 0.f;
        }
    }
    if (r_lo >= r_hi) return;
    const uint16_t* mk = a.masks[y] + (size_t)(nh - 1) * mask_rowtiles(M) * NTm * 64 +
                         (size_t)(n0 >> 5) * 64 + lane;
    const size_t mstride = (size_t)NTm * 64;
    const float* dyp = a.dy[y];
    const int ld_dy = a.ld_dy, ld_in = a.ld_in;
    const float* xin = a.in + a.in_col;
    // raw loads of a 32-row tile (A operands: lane l32 = row, h = k; the lane's 2 mask words),
    // in tile order through running per-lane pointers (a 64-bit add per stream and tile: the
    // address math is VALU, which the f32 MFMA waits for); a partial last tile reads clamped rows,
    // and what does not exist is zeroed where it is used
    const int gk = h < d_out ? h : 0, xk0 = h < d_in ? h : 0, xk1 = 2 + h < d_in ? 2 + h : 0;
    struct Raw {
        float g, x0, x1;
        uint32_t m0, m1;
    };
    const float* gp = dyp + (r_lo + l32) * ld_dy + gk;
    const float* xp = xin + (r_lo + l32) * ld_in;
    const uint16_t* mp = mk + (size_t)(r_lo >> 5) * mstride;
    const int64_t gstep = 32 * (int64_t)ld_dy, xstep = 32 * (int64_t)ld_in;
    int64_t rl = r_lo;  // first row of the next tile to load
    auto load = [&](int64_t) {
        Raw v;
        if (rl + 32 <= r_hi) {
            v.g = *gp;
            v.x0 = xp[xk0];
            v.x1 = xp[xk1];
            v.m0 = mp[0];
            v.m1 = mp[64];
        } else {  // rows past r_hi read row r_lo (the values are not used)
            const bool ok = rl + l32 < r_hi;
            const float* g = ok ? gp : dyp + r_lo * ld_dy + gk;
            const float* x = ok ? xp : xin + r_lo * ld_in;
            v.g = *g;
            v.x0 = x[xk0];
            v.x1 = x[xk1];
            v.m0 = mp[0];
            v.m1 = mp[64];
        }
        gp += gstep;
        xp += xstep;
        mp += mstride;
        rl += 32;
        return v;
    };
    // operand MFMAs of one tile (results in the C layout, masked later by finish())
    // the h_0 tiles start at the (scaled) bias of their column, set by VALU: the same C operand
    // the K = 2 bias MFMA of (1, 0) x (b, 0) produced (exactly b), one f32 MFMA fewer per column
    // half and tile; inputs 2, 3 only exist for d_in > 2 (the actor has 2)
    float bc[2];  // set below, after the scales
    const bool x23 = d_in > 2;
    auto issue = [&](int64_t rt, const Raw& v, f32x16 (&P)[2], f32x16 (&Q)[2]) {
        const bool ok = rt + l32 < r_hi && h < d_out;  // rows past r_hi: dz = 0, add nothing
        const float g = ok ? v.g : 0.f;
        const float x0 = h < d_in ? v.x0 : 0.f, x1 = 2 + h < d_in ? v.x1 : 0.f;
        const f32x16 zero = {};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            P[i] = mfma(g, wob[i], zero);
            f32x16 b;
#pragma unroll
            for (int e = 0; e < 16; ++e) b[e] = bc[i];
            Q[i] = mfma(x0, w0b[i][0], b);
        }
        if (x23) {
#pragma unroll
            for (int i = 0; i < 2; ++i) Q[i] = mfma(x1, w0b[i][1], Q[i]);
        }
    };
    // ReLU derivative of the top layer on P (bit e of the lane's word as an all-ones mask) and
    // the layer-0 ReLU on Q (an integer max of the bit pattern: one v_max_i32)
    auto finish = [&](const Raw& v, f32x16 (&P)[2], f32x16 (&Q)[2]) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            // v_bfe_i32 of one bit: 0 or all ones
            P[0][e] = __int_as_float(__float_as_int(P[0][e]) & __builtin_amdgcn_sbfe((int)v.m0, e, 1));
            P[1][e] = __int_as_float(__float_as_int(P[1][e]) & __builtin_amdgcn_sbfe((int)v.m1, e, 1));
            Q[0][e] = __int_as_float(max(__float_as_int(Q[0][e]), 0));
            Q[1][e] = __int_as_float(max(__float_as_int(Q[1][e]), 0));
        }
    };
    // per 32-row tile: the operand MFMAs, their ReLU epilogue, then the tile's two 16-deep k steps
    // of the fp16 product (the partner wave on the SIMD keeps the matrix pipe busy while this one
    // waits for its operand MFMAs; double-buffering the operand tiles would not fit the 256
    // registers of two waves per SIMD next to the split fragments). The raw loads run two tiles
    // ahead.
    Raw cur = load(r_lo);
    Raw nxt = cur;
    if (r_lo + 32 < r_hi) nxt = load(r_lo + 32);
    // (the first two tiles' loads are in flight under the bound pre-pass)
    // fp16 operand scales (mlp_common.h), folded into the operand MFMAs' constants (a power of two
    // commutes with every rounding of the f32 chains): P column tile i by 2^ep[i] from the bound
    // sum_d max|g_d| |Wo[d][n]| (max over the tile's 32 n), Q column k by 2^eq[j] from h0_bound
    int ep[2], eq[2];
    {
        float G[2], X[4];
        WG_MARK(1, 2);
        row_maxima(a, y, r_lo, r_hi, G, X);
        WG_MARK(1, 3);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float b = G[h] * fabsf(wob[i]);
            b += __shfl_xor(b, 32, 64);
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) b = fmaxf(b, __shfl_xor(b, m, 64));
            ep[i] = pow2_exp(b);
            wob[i] = ldexpf(wob[i], ep[i]);
            float wm = fmaxf(fmaxf(fabsf(w0b[i][0]), fabsf(w0b[i][1])), fabsf(bob[i]));
            wm = fmaxf(wm, __shfl_xor(wm, 32, 64));
            eq[i] = cap_exp_finite(pow2_exp(h0_bound(X, w0b[i][0], w0b[i][1], bob[i])), wm);
            w0b[i][0] = ldexpf(w0b[i][0], eq[i]);
            w0b[i][1] = ldexpf(w0b[i][1], eq[i]);
            bob[i] = ldexpf(bob[i], eq[i]);
            bc[i] = bob[i] + __shfl_xor(bob[i], 32, 64);  // the column's scaled bias, both halves
        }
    }
    for (int64_t rt = r_lo; rt < r_hi; rt += 32) {
        Raw nn = nxt;
        if (rt + 64 < r_hi) nn = load(rt + 64);
        f32x16 P[2], Q[2];
        issue(rt, cur, P, Q);
        finish(cur, P, Q);
        // registers 8s .. 8s+7 of the C-layout operands are k step s (rows 16s + 8(j>>2) + 4h +
        // (j&3), the same for P and Q), each (already scaled) split into two fp16 planes right
        // before its three products
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            Split2 sp[2], sq[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float vp[8], vq[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    vp[t] = P[i][8 * s2 + t];
                    vq[t] = Q[i][8 * s2 + t];
                }
                sp[i] = split2_8(vp);
                sq[i] = split2_8(vq);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_x3s(sp[i], sq[j], acc[i][j]);
        }
        cur = nxt;
        nxt = nn;
    }
    WG_MARK(1, 4);
    // unscale: tile (i, j) by 2^-(ep[i] + eq[j]) (eq per lane column), exact
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = ldexpf(acc[i][j][e], -(ep[i] + eq[j]));
}

// ---- the factored form for 2-hidden-layer networks (the bench shape) ----
// With e the forward's ReLU bit of the top hidden layer and g_d = dL/dy_d,
//   dz_1[r][n] = e[r][n] sum_d g_d[r] Wo[d][n]        (robot.py:355-363 autograd, d < d_out)
//   dW_1[n][k] = sum_r dz_1[r][n] h_0[r][k] = sum_d Wo[d][n] S_d[n][k],
//   S_d[n][k]  = sum_r e[r][n] Q_d[r][k],   Q_d[r][k] = g_d[r] h_0[r][k].
// The A operand of S_d is the ReLU bit itself, exact in fp16 (as 2.0, the 0.5 goes into Wo; 8
// bits of a mask word become an A fragment by one 16-B read of a 256-entry LDS table — fp16 2.0
// and bf16 2.0 share the bit pattern 0x4000), and only the B operand Q_d is split: scaled by a
// power of two (h_0 per column k into [2^6, 2^7) through the layer-0 constants, g_d per wave into
// [2^7, 2^8) from the wave's max |g_d|) and cut into two fp16 planes, so the product carries f32
// accuracy with 2 MFMAs per 16-deep k step and 32 x 32 tile (the three-plane bf16 form: 3), and
// nothing per element on the n side. That frees a wave to own NI * KH = 8 blocks of 32 x 32 at
// D = 1 — the twin critics — for 128 accumulator registers: all 8 along n (256 x 32) at hp 256,
// so that no other workgroup of the launch forms the same Q; 128 x 64 at hp 128.


// GV: dy rows packed (ld_dy = D) and 16-B aligned (float4 loads at fixed offsets); XV: x rows of 4
// floats, 16-B aligned (one float4 load per row). Both are launch-uniform: the full-tile loop is
// compiled per form, with running row pointers and no per-tile branch on the layout.
// KH: 32-column halves of the k side per wave (tile NI*32 x KH*32; NI * KH = 8 at D = 1).
template <int NI, int D, int KH, bool GV, bool XV>
NAV_DEV void wgrad_rows_fact(const WgradArgs& a, int y, int n0, int k0, int64_t r_lo,
                             int64_t r_hi, const char* tab, f32x16 (&out)[NI][KH]) {
    const MlpDev& net = a.net[y];
    const int hp = net.hp, d_in = net.d_in;
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int64_t M = a.M;
    const int NTm = hp >> 5;
    f32x16 acc[D][NI][KH];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < KH; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[d][i][j][e] = 0.f;
    // h_0 = relu(x . W0^T + b0) by f32 MFMAs in the C layout, where lane (l32, h) register e
    // holds row acc_row(e, h) of column l32. Constant B operands: W0 columns (k = h, then 2 + h),
    // and the bias through a K = 2 MFMA of (1, 0) x (b, 0), so the C tile starts at b exactly and
    // h_0 accumulates in layer0_unit's order b + x0 w0 + x1 w1 + x2 w2 + x3 w3
    float w0b[KH][2], bob[KH];
    {
        const float* W0 = net.params + net.w_off[0];
        const float* bb = net.params + net.b_off[0];
#pragma unroll
        for (int j = 0; j < KH; ++j) {
            const int c = k0 + 32 * j + l32;
            w0b[j][0] = h < d_in ? W0[c * d_in + h] : 0.f;
            w0b[j][1] = 2 + h < d_in ? W0[c * d_in + 2 + h] : 0.f;
            bob[j] = h == 0 ? bb[c] : 0.f;
        }
    }
    int eh[KH], eg[D];  // the fp16 operand scales (below, under the first tile's loads)
    float sg[D];
    float bcj[KH];     // the scaled bias of the lane's column per half (below, with the scales)
    const bool x23 = d_in > 2;
    const size_t mstride = (size_t)NTm * 64;
    const uint16_t* mp = a.masks[y] + (size_t)mask_rowtiles(M) * mstride +  // layer 1's bits
                         (size_t)(n0 >> 5) * 64 + lane + (size_t)(r_lo >> 5) * mstride;
    const float* dyp = a.dy[y];
    const int ld_dy = a.ld_dy, ld_in = a.ld_in;
    const int xk0 = h < d_in ? h : 0, xk1 = 2 + h < d_in ? 2 + h : 0;
    // the tile's own A operands (x row of lane l32, inputs k = h and 2 + h) and the lane's NI
    // mask words; the main loop keeps the next full tile's in flight
    // (NI = 8: two 16-bit mask words per register, tile 2u in the low half, so the current and the
    // prefetched set hold 8 registers instead of 16; byte 2 (i & 1) + s2 of m[i >> 1] is k step s2)
    constexpr bool MP = NI == 8;
    constexpr int NM = MP ? NI / 2 : NI;
    struct Raw {
        float x0, x1;
        uint32_t m[NM];
    };
    auto load_masks = [&](const uint16_t* m, Raw& v) {
#pragma unroll
        for (int u = 0; u < NM; ++u)
            v.m[u] = MP ? (uint32_t)m[2 * u * 64] | ((uint32_t)m[(2 * u + 1) * 64] << 16)
                        : (uint32_t)m[u * 64];
    };
    // the x row as one 16-B load when it is 4 aligned floats (both lane halves read the row)
    const bool xrow4 = d_in == 4 && (ld_in & 3) == 0 && (((uintptr_t)(a.in + a.in_col)) & 15) == 0;
    auto load_raw = [&](int64_t rt, Raw& v) {
        const int64_t rx = rt + l32 < r_hi ? rt + l32 : r_lo;  // absent rows read row r_lo
        const float* x = a.in + a.in_col + rx * ld_in;
        if (xrow4) {
            const float4 u = *reinterpret_cast<const float4*>(x);
            v.x0 = h ? u.y : u.x;
            v.x1 = h ? u.w : u.z;
        } else {
            v.x0 = x[xk0];
            v.x1 = x[xk1];
        }
        load_masks(mp + (size_t)((rt - r_lo) >> 5) * mstride, v);
    };
    // one 32-row tile: h_0 by the f32 MFMAs, Q_d = relu(h_0) g_d split per k step, 2 MFMAs per
    // (i, j, d) and step. gs[s2][d][t]: g_d (scaled) of the row of register e = 8 s2 + t
    auto tile = [&](const Raw& cur, const float (&gs)[2][D][8]) {
        const float x0 = h < d_in ? cur.x0 : 0.f, x1 = 2 + h < d_in ? cur.x1 : 0.f;
        // one 32-column half j of the k side at a time (16 registers of h_0 live)
#pragma unroll
        for (int j = 0; j < KH; ++j) {
            // the C operand starts at the column's scaled bias (exactly what the K = 2 bias MFMA
            // of (1, 0) x (b, 0) produced), set by VALU: one f32 MFMA fewer per half and tile
            f32x16 Z;
#pragma unroll
            for (int e = 0; e < 16; ++e) Z[e] = bcj[j];
            Z = mfma(x0, w0b[j][0], Z);
            if (x23) Z = mfma(x1, w0b[j][1], Z);
            // registers 8s .. 8s+7 of the C layout are k step s (rows 16s + 8(t>>2) + 4h +
            // (t&3)), the same rows as bits 8s .. 8s+7 of the lane's mask words
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    float q[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        q[t] = __int_as_float(max(__float_as_int(Z[8 * s2 + t]), 0)) * gs[s2][d][t];
                    const Split2 sq = split2_8(q);
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        // the fragment of byte s2 of the mask word, read from the table right
                        // before its 3 MFMAs (the opaque offset keeps the compiler from holding
                        // all NI x 2 fragments live across the passes over j)
                        uint32_t ta = MP ? ((cur.m[i >> 1] >> (16 * (i & 1) + 8 * s2)) & 0xFFu) << 4
                                         : (s2 == 0 ? cur.m[i] << 4 : cur.m[i] >> 4) & 0xFF0u;
                        asm volatile("" : "+v"(ta));
                        const f16x8 pi = *reinterpret_cast<const f16x8*>(tab + ta);
                        acc[d][i][j] = mfma_h(pi, sq.l, acc[d][i][j]);
                        acc[d][i][j] = mfma_h(pi, sq.h, acc[d][i][j]);
                    }
                }
        }
    };
    const int64_t r_full = r_lo + ((r_hi - r_lo) & ~(int64_t)31);
    constexpr int LDG = GV ? D : 0;  // the compile-time dy row stride of the GV form
    const int ldg = GV ? LDG : ld_dy;
    // the g values of rows rt + 4h + 16 s2 + 8 qq + t (register e = 8 s2 + 4 qq + t of the C
    // layout) from the row pointer g0 = dy + (rt + 4h) ldg
    auto load_g_at = [&](const float* gp, float (&gs)[2][D][8]) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                const float* g = gp + (16 * s2 + 8 * qq) * ldg;
                if (GV && D == 1) {
                    const float4 u = *reinterpret_cast<const float4*>(g);
                    gs[s2][0][4 * qq] = u.x; gs[s2][0][4 * qq + 1] = u.y;
                    gs[s2][0][4 * qq + 2] = u.z; gs[s2][0][4 * qq + 3] = u.w;
                } else if (GV) {
                    const float4 u0 = *reinterpret_cast<const float4*>(g);
                    const float4 u1 = *reinterpret_cast<const float4*>(g + 4);
                    gs[s2][0][4 * qq] = u0.x; gs[s2][D - 1][4 * qq] = u0.y;
                    gs[s2][0][4 * qq + 1] = u0.z; gs[s2][D - 1][4 * qq + 1] = u0.w;
                    gs[s2][0][4 * qq + 2] = u1.x; gs[s2][D - 1][4 * qq + 2] = u1.y;
                    gs[s2][0][4 * qq + 3] = u1.z; gs[s2][D - 1][4 * qq + 3] = u1.w;
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int d = 0; d < D; ++d) gs[s2][d][4 * qq + t] = g[t * ldg + d];
                }
            }
    };
    // the g scales on the loaded values (D = 2; D = 1 folds them into the layer-0 constants)
    auto scale_g = [&](float (&gs)[2][D][8]) {
        if (D == 1) return;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int t = 0; t < 8; ++t) gs[s2][d][t] *= sg[d];
    };
    // full tiles: running per-lane pointers (x row, mask words, g rows), every row in range, so no
    // clamp; d_out = 1 loads its g values one tile ahead with the rest (d_out = 2 at the tile: its
    // 32 prefetched values do not fit the registers)
    constexpr bool GPF = D == 1;
    const int64_t nfull = (r_full - r_lo) >> 5;
    const float* xq = a.in + a.in_col + (r_lo + l32) * (int64_t)ld_in;
    const uint16_t* mq = mp;
    const float* gq = dyp + (r_lo + 4 * h) * (int64_t)ldg;
    const int64_t xstep = 32 * (int64_t)ld_in, gstep = 32 * (int64_t)ldg;
    auto load_full = [&](Raw& v, float (&gs)[2][D][8]) {
        if (XV) {
            const float4 u = *reinterpret_cast<const float4*>(xq);
            v.x0 = h ? u.y : u.x;
            v.x1 = h ? u.w : u.z;
        } else {
            v.x0 = xq[xk0];
            v.x1 = xq[xk1];
        }
        load_masks(mq, v);
        if (GPF) load_g_at(gq, gs);
        xq += xstep;
        mq += mstride;
        gq += gstep;
    };
    Raw c0, c1;
    float g0[2][D][8], g1[2][D][8];
    if (nfull > 0) load_full(c0, g0);
    // the scales, computed under the first tile's loads: h_0 column half j by 2^eh[j] (folded into
    // the layer-0 constants: a power of two commutes with the fma chain's roundings), g_d by
    // 2^eg[d] (D = 1: folded into the same constants, so the g rows are used as loaded; D = 2:
    // applied to the loaded g values)
    {
        float G[2], X[4];
        WG_MARK(0, 2);
        row_maxima(a, y, r_lo, r_hi, G, X);
        WG_MARK(0, 3);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            eg[d] = pow2_exp_to(G[d], 8);
            sg[d] = D == 1 ? 1.f : ldexpf(1.f, eg[d]);
        }
        // per 32-column half (wave-uniform, scalar registers: the 128-accumulator program has no
        // vector register to spare)
#pragma unroll
        for (int j = 0; j < KH; ++j) {
            eh[j] = __builtin_amdgcn_readfirstlane(
                pow2_exp_to(wave_max_abs(h0_bound(X, w0b[j][0], w0b[j][1], bob[j])), 7));
            // (the sum capped at 2^120: Z = h_0 2^eh stays finite for every finite h_0 bound)
            if (D == 1) eh[j] = min(max(eh[j] + eg[0], -126), 120);
            eh[j] = __builtin_amdgcn_readfirstlane(cap_exp_finite(
                eh[j], wave_max_abs(fmaxf(fmaxf(fabsf(w0b[j][0]), fabsf(w0b[j][1])),
                                          fabsf(bob[j])))));
            w0b[j][0] = ldexpf(w0b[j][0], eh[j]);
            w0b[j][1] = ldexpf(w0b[j][1], eh[j]);
            bob[j] = ldexpf(bob[j], eh[j]);
            bcj[j] = bob[j] + __shfl_xor(bob[j], 32, 64);  // the column's scaled bias, both halves
        }
        if (D == 1) eg[0] = 0;
    }
    for (int64_t t = 0; t < nfull; ++t) {
        if (t + 1 < nfull) load_full(c1, g1);
        if (!GPF) load_g_at(dyp + (r_lo + 32 * t + 4 * h) * (int64_t)ldg, g0);
        scale_g(g0);
        tile(c0, g0);
        c0 = c1;
        if (GPF) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int d = 0; d < D; ++d)
#pragma unroll
                    for (int e = 0; e < 8; ++e) g0[s2][d][e] = g1[s2][d][e];
        }
    }
    WG_MARK(0, 4);
    if (r_full < r_hi) {  // the last, partial tile of the rows (M % 32 rows)
        Raw cur;
        load_raw(r_full, cur);
        float gs[2][D][8];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t r = r_full + acc_row(e, h);
#pragma unroll
            for (int d = 0; d < D; ++d) gs[e >> 3][d][e & 7] = r < r_hi ? dyp[r * ld_dy + d] * sg[d] : 0.f;
        }
        tile(cur, gs);
    }
    // dW tile = sum_d (Wo[d][n] / 2) S_d: register e of tile (i, j) is row n = n0 + 32 i +
    // acc_row(e, h)
    const float* Wo = net.params + net.w_off[net.n_hidden];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        // NI = 8: two column tiles' Wo loads at a time (all 32 float4 loads hoisted above the
        // products cost 17 spilled registers next to the 128 accumulators)
        if (NI == 8 && i > 0 && i % 2 == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + 32 * i + 8 * q + 4 * h;
            float4 wv[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float* w = Wo + d * hp + n;
                wv[d] = make_float4(w[0], w[1], w[2], w[3]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int e = 4 * q + t;
#pragma unroll
                for (int j = 0; j < KH; ++j) {
                    const float w0 = (t == 0 ? wv[0].x : t == 1 ? wv[0].y : t == 2 ? wv[0].z : wv[0].w) * 0.5f;
                    float v = w0 * ldexpf(acc[0][i][j][e], -(eh[j] + eg[0]));
                    if (D > 1) {
                        const float w1 = (t == 0 ? wv[D - 1].x : t == 1 ? wv[D - 1].y
                                          : t == 2 ? wv[D - 1].z : wv[D - 1].w) * 0.5f;
                        v = fmaf(w1, ldexpf(acc[D - 1][i][j][e], -(eh[j] + eg[D - 1])), v);
                    }
                    out[i][j][e] = v;
                }
            }
        }
    }
}

// The NI x KH blocks of each wave summed across the 8 waves through LDS (R slots of NI*32 x KH*32
// floats in 128 KB: waves w and w + R share slot w % R, in wave order) and written as one slab tile.
// Slot layout: per 32 x 32 block (i, j) and lane, the lane's 16 accumulator values contiguous
// (16-B LDS accesses, 4 per block instead of 16 single-dword ones), the 4 chunks of a lane
// rotated by (lane >> 2) & 3 so the 8 lanes of one LDS cycle hit distinct banks. The final pass
// gives wave w the blocks w, w + 8, ...: 16 values per lane summed over the slots in slot order
// (the same order as p_0 + p_R + p_1 + ... of a row-major slot), each stored to 32 consecutive
// columns of a slab row per lane half.
template <int NI, int KH>
NAV_DEV void wgrad_reduce_write(const WgradArgs& a, int y, int split, int L, int n0, int k0,
                                const f32x16 (&acc)[NI][KH], float* red) {
    constexpr int T = NI * 32 * 32 * KH;
    constexpr int R = (WG_WAVES * WG_TILE * WG_TILE) / T < WG_WAVES
                          ? (WG_WAVES * WG_TILE * WG_TILE) / T : WG_WAVES;
    const MlpDev& net = a.net[y];
    const int hp = net.hp;
    const int wv = wave_id(), lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    const int rot = (lane >> 2) & 3;
    float4* mine = reinterpret_cast<float4*>(red + (wv % R) * T);
#pragma unroll
    for (int round = 0; round < WG_WAVES / R; ++round) {
        if (wv / R == round) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < KH; ++j) {
                    float4* p = mine + ((i * KH + j) * 64 + lane) * 4;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float4 v = make_float4(acc[i][j][4 * c], acc[i][j][4 * c + 1],
                                               acc[i][j][4 * c + 2], acc[i][j][4 * c + 3]);
                        if (round) {
                            const float4 o = p[c ^ rot];
                            v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
                        }
                        p[c ^ rot] = v;
                    }
                }
        }
        __syncthreads();
    }
    float* o = a.slabs[y] + (int64_t)split * hidden_w_count(net) + (int64_t)(L - 1) * hp * hp;
    const float4* slots = reinterpret_cast<const float4*>(red);
    for (int b = wv; b < NI * KH; b += WG_WAVES) {
        const int i = b / KH, j = b % KH;
        float v[16];
#pragma unroll
        for (int w = 0; w < R; ++w) {
            const float4* p = slots + (size_t)w * (T / 4) + (b * 64 + lane) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 u = p[c ^ rot];
                if (w == 0) {
                    v[4 * c] = u.x; v[4 * c + 1] = u.y; v[4 * c + 2] = u.z; v[4 * c + 3] = u.w;
                } else {
                    v[4 * c] += u.x; v[4 * c + 1] += u.y; v[4 * c + 2] += u.z; v[4 * c + 3] += u.w;
                }
            }
        }
        const int col = k0 + 32 * j + l32;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = n0 + 32 * i + acc_row(e, h);
            if (n < hp && col < hp) o[(int64_t)n * hp + col] = v[e];
        }
    }
}

// One workgroup's tile job: network y, hidden layer L, output tile (n0.., k0..), row split.
// Workgroups b of a grid of `total`: nets x tile jobs x splits. Block order is XCD-grouped
// (blocks b and b + 8 share an XCD's L2): the tile jobs of one (net, split) — which read the same
// rows — are consecutive in the virtual order v and land on one XCD.
struct TileJob {
    int y, job, split, L, n0, k0;
};
NAV_DEV TileJob wgrad_job(const WgradArgs& a, int b, int total) {
    const int v = (total % 8 == 0) ? (b % 8) * (total / 8) + b / 8 : b;
    const int grp = v / a.n_hid, TT = a.TT, TN = a.TN;
    TileJob t;
    t.job = v % a.n_hid;
    t.y = grp / a.splits;
    t.split = grp % a.splits;
    t.L = t.job / (TN * TT) + 1;
    t.n0 = ((t.job % (TN * TT)) / TT) * a.tn;
    t.k0 = (t.job % TT) * a.tk;
    return t;
}

// split s's rows for wave wv: [r_lo, r_hi). Waves w and w + 4 share a SIMD, and its arbiter
// issues the older wave first: with equal rows the second wave of every SIMD reached the LDS
// reduce ~9 k cycles after the first and ran that tail alone (profiles/r05z). `skew` rows (a
// multiple of 32: whole tiles) move from wave w + 4 to wave w, so the pair finishes together.
NAV_DEV void wave_rows(const WgradArgs& a, int split, int wv, int64_t skew, int64_t& r_lo,
                       int64_t& r_hi) {
    const int64_t M = a.M;
    const int64_t s_lo = (int64_t)split * a.per_split < M ? (int64_t)split * a.per_split : M;
    const int64_t s_hi = s_lo + a.per_split < M ? s_lo + a.per_split : M;
    const int64_t pa = a.per_wave + skew, pb = a.per_wave - skew;  // waves 0-3, 4-7
    const int64_t off = wv < WG_WAVES / 2 ? wv * pa : (WG_WAVES / 2) * pa + (wv - WG_WAVES / 2) * pb;
    const int64_t len = wv < WG_WAVES / 2 ? pa : pb;
    r_lo = s_lo + off < s_hi ? s_lo + off : s_hi;
    r_hi = r_lo + len < s_hi ? r_lo + len : s_hi;
}

template <int NI, int D, int KH>
NAV_DEV void wgrad_tile_fact(const WgradArgs& a, const TileJob& t, float* smem, uint4* tab) {
    WG_MARK(0, 0);
    // the bits -> A fragment table (a static LDS array: its address is a constant, so a fragment
    // read is one ds_read_b128 at the entry's offset): entry b, dword d holds fp16 2.0 (0x4000)
    // in its low half when bit 2d of b is set and in its high half when bit 2d + 1 is
    if (threadIdx.x < 256) {
        const uint32_t b = threadIdx.x;
        uint32_t w[4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
            w[d] = ((b >> (2 * d)) & 1u ? 0x4000u : 0u) | ((b >> (2 * d + 1)) & 1u ? 0x40000000u : 0u);
        tab[b] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    WG_MARK(0, 1);
    int64_t r_lo, r_hi;
    wave_rows(a, t.split, wave_id(), a.skew, r_lo, r_hi);
    f32x16 out[NI][KH];
    const char* tb = reinterpret_cast<const char*>(tab);
    const bool gv = a.ld_dy == D && ((uintptr_t)a.dy[t.y] & 15) == 0;
    const bool xv = a.net[t.y].d_in == 4 && (a.ld_in & 3) == 0 &&
                    ((uintptr_t)(a.in + a.in_col) & 15) == 0;
    if (gv && xv) wgrad_rows_fact<NI, D, KH, true, true>(a, t.y, t.n0, t.k0, r_lo, r_hi, tb, out);
    else if (gv) wgrad_rows_fact<NI, D, KH, true, false>(a, t.y, t.n0, t.k0, r_lo, r_hi, tb, out);
    else if (xv) wgrad_rows_fact<NI, D, KH, false, true>(a, t.y, t.n0, t.k0, r_lo, r_hi, tb, out);
    else wgrad_rows_fact<NI, D, KH, false, false>(a, t.y, t.n0, t.k0, r_lo, r_hi, tb, out);
    WG_MARK(0, 5);
    wgrad_reduce_write<NI, KH>(a, t.y, t.split, t.L, t.n0, t.k0, out, smem);
    WG_MARK(0, 6);
}

// The tile job's partial over its split's rows, written as one slab tile (8 waves' partials
// summed in wave order). GEN (k_wgrad_gen, networks of >= 3 hidden layers, whose tiles never take
// the MFMA-operand path): the generic rows only, with their saved rows loaded ahead (RA)
template <bool GEN>
NAV_DEV void wgrad_tile(const WgradArgs& a, const TileJob& t, float* smem) {
    WG_MARK(1, 0);
    const int y = t.y, split = t.split, L = t.L, n0 = t.n0, k0 = t.k0;
    const int nh = a.net[y].n_hidden;
    const int wv = wave_id();
    const bool pr = L == nh - 1, qr = L == 1;
    const bool full = n0 + WG_TILE <= a.net[y].hp && k0 + WG_TILE <= a.net[y].hp;
    const bool opnd = pr && qr && full;  // the MFMA-operand path (32-row tiles: skew allowed)
    int64_t r_lo, r_hi;
    wave_rows(a, split, wv, opnd ? a.skew : 0, r_lo, r_hi);
    float* red = smem;                                          // [8][64][64]
    float* stage = smem + WG_WAVES * WG_TILE * WG_TILE + wv * 2 * WG_STAGE_FLOATS;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    if constexpr (GEN) {
        if (pr && qr) wgrad_rows<true, true, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else if (pr) wgrad_rows<true, false, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else if (qr) wgrad_rows<false, true, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else wgrad_rows<false, false, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
    } else {
        if (opnd) wgrad_rows_mfma(a, y, n0, k0, r_lo, r_hi, acc);
        else if (pr && qr) wgrad_rows<true, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else if (pr) wgrad_rows<true, false>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else if (qr) wgrad_rows<false, true>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
        else wgrad_rows<false, false>(a, y, L, n0, k0, r_lo, r_hi, stage, acc);
    }
    // the 8 partial tiles meet in LDS, summed in wave order
    WG_MARK(1, 5);
    wgrad_reduce_write<2, 2>(a, y, split, L, n0, k0, acc, red);
    WG_MARK(1, 6);
}

}  // namespace
