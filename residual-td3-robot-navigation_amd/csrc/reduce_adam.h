// reduce_adam.h — the device code of the learner's optimizer side: the argument structs of the
// image packer, the gradient reduce (+ Adam, + the soft updates), multi-net Adam and Polyak, and
// the bodies their kernels (learner_kernels.hip, learner_pop.hip) wrap. The image packer's
// statements are pack_img_body.inc.
#pragma once
#include "mlp_common.h"

namespace {

// ---------------- optimizer / target update, refreshing the packed images ----------------
struct PackInfo {
    int hp, n_hidden, d_out;
    int64_t w_off[kMaxLayers];
    float* packed;
};

// The fp16 B images (mlp_common.h) of every hidden x hidden weight of up to 8 networks, rebuilt
// from the f32 parameters after each writer (Adam, Polyak, pack). One workgroup per (network,
// hidden layer, image, 16-column group): thread (c = t & 15, kq = t >> 4) holds the 16 values
// B[16 kq .. 16 kq + 15][16 g + c] in registers; the column's max |B| meets in LDS, then every
// thread writes its two 8-k entries of both planes and the kq = 0 thread the exponent e_n. The
// forward image's column n is W_L's row n (B[k][n] = W_L[n][k]: float4 reads along the row), the
// backward image's is W_L's column n (B[k][n] = W_L[k][n]: 16 lanes on 64 consecutive bytes).
// hp / 16 <= 16 k chunks: one load round trip and no second pass over W.
// For d_out = 1 the TOP hidden layer's backward image holds Wt[k][n] = Wo[k] * W_L[k][n] (f32
// products) instead of W_L: the row backward's top GEMM then takes the forward's ReLU bits as
// its exact fp16 A operand and applies dL/dq per row after the sum (mlp_rows.h gemm_bits).
struct PackJob {
    const float* p;
    PackInfo pk;
};
struct PackArgs {
    PackJob j[8];
    int n, per_net, cg;
};

NAV_DEV float adam1(float& p, float g, float& m, float& v, float b1w, float b2, float omb2,
                    float eps, float step_size, float bc2s) {
    // torch 2.10 _single_tensor_adam: m.lerp_(g, 1-b1); v.mul_(b2).addcmul_(g, g, 1-b2);
    // denom = v.sqrt()/bc2_sqrt + eps; p.addcdiv_(m, denom, -step_size)
    m = fmaf(b1w, g - m, m);
    v = v * b2 + (omb2 * g) * g;
    const float denom = sqrtf(v) / bc2s + eps;
    p = p + (-step_size) * (m / denom);
    return p;
}

// ---------------- gradient reduce (+ fused Adam) ----------------
// grad = hidden-W entries: sum of the weight-gradient split slabs (block = 64 float4 columns x 4
// split groups, the group sums added in order through LDS); every other entry: sum of the
// per-row-block edge slabs (one wave per float4, lanes take blocks b = lane, lane + 64, ..., a
// fixed xor tree adds the lanes). Deterministic: the same order on every run. With ADAM the
// finished gradient goes straight into torch's Adam update (robot.py:236-239) of the parameter
// it belongs to and the packed MFMA images are refreshed; up to 2 networks per launch.
// robot.py:293-310 soft update of up to 4 (target, source) pairs in one launch
struct PolyPair {
    float4* t;
    const float4* s;
    int64_t n4;
};
struct PolyArgs {
    PolyPair q[4];
    int n;
    int64_t total4;
    float omt, tau;
};

struct RedNet {
    MlpDev net;
    const float4* hs;
    const float4* es;
    float4* grad;  // nullable with ADAM
    float4* p;
    float4* m;
    float4* v;
    float step_size, bc2s;
    int nbh, nbe;
    float4* tgt;   // nullable: this net's target, soft-updated from the new parameters
};

struct RedArgs {
    RedNet n[2];
    int splits;
    int64_t nblk;
    float b1w, b2, omb2, eps;
    // the soft updates of the launch (robot.py:283-285): the nets' own targets in red_out, the
    // extra (target, source) pairs by the blocks past the reduce blocks
    PolyArgs poly;
    int red_blocks;
};

// Adam on the float4 of parameters at flat4 with its finished gradient g and the net's own
// target (when soft-updated in the launch); the packed images follow in k_pack_img
// (POP, the population form: Adam's constants, the step's step size and sqrt(1 - b2^t) come with
// the launch, `st`, instead of the table entry, which then holds none of them)
struct AdamStep {
    float step_size, bc2s, b1w, b2, omb2, eps;
};
template <bool POP>
NAV_DEV void adam_out(const RedArgs& a, const RedNet& rn, int64_t flat4, float4 g,
                      const AdamStep& st) {
    float4 pp = rn.p[flat4], mm = rn.m[flat4], vv = rn.v[flat4];
    if constexpr (POP) {
        adam1(pp.x, g.x, mm.x, vv.x, st.b1w, st.b2, st.omb2, st.eps, st.step_size, st.bc2s);
        adam1(pp.y, g.y, mm.y, vv.y, st.b1w, st.b2, st.omb2, st.eps, st.step_size, st.bc2s);
        adam1(pp.z, g.z, mm.z, vv.z, st.b1w, st.b2, st.omb2, st.eps, st.step_size, st.bc2s);
        adam1(pp.w, g.w, mm.w, vv.w, st.b1w, st.b2, st.omb2, st.eps, st.step_size, st.bc2s);
    } else {
        adam1(pp.x, g.x, mm.x, vv.x, a.b1w, a.b2, a.omb2, a.eps, rn.step_size, rn.bc2s);
        adam1(pp.y, g.y, mm.y, vv.y, a.b1w, a.b2, a.omb2, a.eps, rn.step_size, rn.bc2s);
        adam1(pp.z, g.z, mm.z, vv.z, a.b1w, a.b2, a.omb2, a.eps, rn.step_size, rn.bc2s);
        adam1(pp.w, g.w, mm.w, vv.w, a.b1w, a.b2, a.omb2, a.eps, rn.step_size, rn.bc2s);
    }
    rn.p[flat4] = pp;
    rn.m[flat4] = mm;
    rn.v[flat4] = vv;
    if (rn.tgt) {  // robot.py:309 on the parameter just stepped (k_polyak's expression)
        float4 t = rn.tgt[flat4];
        t.x = t.x * a.poly.omt + pp.x * a.poly.tau;
        t.y = t.y * a.poly.omt + pp.y * a.poly.tau;
        t.z = t.z * a.poly.omt + pp.z * a.poly.tau;
        t.w = t.w * a.poly.omt + pp.w * a.poly.tau;
        rn.tgt[flat4] = t;
    }
}

template <bool ADAM, bool POP>
NAV_DEV void red_out(const RedArgs& a, const RedNet& rn, int64_t flat4, float4 g,
                     const AdamStep& st) {
    if (rn.grad) rn.grad[flat4] = g;
    if (ADAM) adam_out<POP>(a, rn, flat4, g, st);
}

// soft update of element i of the pairs' concatenation (k_polyak_multi's body)
NAV_DEV void polyak_elem(const PolyArgs& a, int64_t i) {
    int64_t j = i;
    int k = 0;
    while (k < a.n - 1 && j >= a.q[k].n4) j -= a.q[k++].n4;
    const PolyPair& q = a.q[k];
    float4 t = q.t[j];
    const float4 s = q.s[j];
    // robot.py:309 target*(1-tau) + source*tau (two products, one sum)
    t.x = t.x * a.omt + s.x * a.tau;
    t.y = t.y * a.omt + s.y * a.tau;
    t.z = t.z * a.omt + s.z * a.tau;
    t.w = t.w * a.omt + s.w * a.tau;
    q.t[j] = t;
}

template <bool ADAM, bool POP>
NAV_DEV void grad_reduce_body(const RedArgs& a, const AdamStep& st) {
    __shared__ float4 part[4][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    int b = blockIdx.x;
    if (b >= a.red_blocks) {  // the extra soft-update pairs (block-uniform)
        for (int64_t i = (int64_t)(b - a.red_blocks) * kBlock + threadIdx.x; i < a.poly.total4;
             i += (int64_t)(gridDim.x - a.red_blocks) * kBlock)
            polyak_elem(a.poly, i);
        return;
    }
    const bool second = b >= a.n[0].nbh + a.n[0].nbe;
    const RedNet& rn = second ? a.n[1] : a.n[0];
    if (second) b -= a.n[0].nbh + a.n[0].nbe;
    const MlpDev& net = rn.net;
    if (b < rn.nbh) {
        const int64_t hw4 = hidden_w_count(net) / 4;
        const int64_t i = (int64_t)b * 64 + c;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < hw4) {
#pragma unroll 4
            for (int k = g; k < a.splits; k += 4) {
                const float4 v = rn.hs[(int64_t)k * hw4 + i];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        part[g][c] = s;
        __syncthreads();
        if (g != 0 || i >= hw4) return;
        float4 r = part[0][c];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            r.x += part[q][c].x; r.y += part[q][c].y; r.z += part[q][c].z; r.w += part[q][c].w;
        }
        const int64_t per = (int64_t)net.hp * net.hp / 4;
        const int L = (int)(i / per) + 1;
        red_out<ADAM, POP>(a, rn, net.w_off[L] / 4 + i % per, r, st);
        return;
    }
    // edge entries: one block = 16 float4 columns x 16 groups of edge blocks; thread (column
    // t & 15, group t >> 4) sums blocks g, g + 16, g + 32, ... in order (a wave instruction reads
    // 4 block rows x 256 contiguous bytes), then the 16 group sums meet in group order in LDS
    const int64_t e4 = edge_count(net) / 4;
    const int ec = threadIdx.x & 15, eg = threadIdx.x >> 4;
    const int64_t o = (int64_t)(b - rn.nbh) * 16 + ec;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o < e4) {
        // 16 loads in flight per trip: a thread's 32 blocks (the bench's 512 / 16 groups) in two
        // memory round trips instead of eight (the launch's critical path)
        const float4* col = rn.es + o;
        int64_t k = eg;
#pragma unroll 1
        for (; k + 240 < a.nblk; k += 256) {
            float4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = col[(k + 16 * u) * e4];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
            }
        }
        for (; k < a.nblk; k += 16) {
            const float4 v = col[k * e4];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    float4* gp = &part[0][0];  // [16 groups][16 columns]
    gp[eg * 16 + ec] = s;
    __syncthreads();
    if (eg != 0 || o >= e4) return;
    float4 r = gp[ec];
#pragma unroll
    for (int q = 1; q < 16; ++q) {
        const float4 v = gp[q * 16 + ec];
        r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    red_out<ADAM, POP>(a, rn, edge_to_flat(net, 4 * o) / 4, r, st);
}

// k_adam_multi's arguments: Adam of up to 2 networks from flat gradients, the soft updates as in
// RedArgs
struct AdamNet {
    float4* p;
    const float4* g;
    float4* m;
    float4* v;
    int64_t n4;
    float step_size, bc2s;
    float4* tgt;  // nullable: this net's target, soft-updated from the new parameters
};
struct AdamArgs {
    AdamNet q[2];
    int n;
    int64_t total4;
    float b1w, b2, omb2, eps, gdiv;
    PolyArgs poly;
    int adam_blocks;
};

}  // namespace
