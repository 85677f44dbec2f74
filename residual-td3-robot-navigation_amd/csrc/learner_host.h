// learner_host.h — what the entry points of learner_kernels.hip and learner_pop.hip share on the
// host (no kernel and no device code): the checks of their arguments, the builders of the kernels'
// argument structs, the split counts and the choice of a weight-gradient launch's kernel form.
#pragma once
#include "pop_host.h"
#include "reduce_adam.h"
#include "wgrad.h"

namespace {

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }
inline int grid_stride_blocks(int64_t n) {
    const int64_t b = (n + kBlock - 1) / kBlock;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

PackInfo pack_info(const MlpDev& d, float* packed) {
    PackInfo pk;
    pk.hp = d.hp;
    pk.n_hidden = d.n_hidden;
    pk.d_out = d.d_out;
    for (int l = 0; l < kMaxLayers; ++l) pk.w_off[l] = l <= d.n_hidden ? d.w_off[l] : 0;
    pk.packed = d.n_hidden > 1 ? packed : nullptr;
    return pk;
}

// The networks whose packed images a launch changed; the entry point rebuilds them (k_pack_img,
// k_pack_img_pop) on the same stream right after the writer.
struct PackSet {
    PackArgs a{};
    bool add(const nav_mlp* net) {
        MlpDev d;
        if (!net || !make_dev(net, &d)) return false;
        if (d.n_hidden < 2) return true;
        if (a.n >= 8) return false;
        a.j[a.n].p = net->params;
        a.j[a.n].pk = pack_info(d, net->packed);
        ++a.n;
        return true;
    }
    // the grid's shape from the jobs: 16-column groups and workgroups per network
    void shape() {
        int hp = 0, nh = 0;
        for (int i = 0; i < a.n; ++i) {
            hp = a.j[i].pk.hp > hp ? a.j[i].pk.hp : hp;
            nh = a.j[i].pk.n_hidden > nh ? a.j[i].pk.n_hidden : nh;
        }
        a.cg = (hp + 15) / 16;
        a.per_net = (nh - 1) * 2 * a.cg;
    }
};

bool red_net(const nav_mlp* net, const float* hs, int splits, const float* es, float* grad,
             RedNet* rn) {
    if (!make_dev(net, &rn->net)) return false;
    if (rn->net.n_hidden > 1 && (!hs || splits < 1)) return false;
    rn->hs = reinterpret_cast<const float4*>(hs);
    rn->es = reinterpret_cast<const float4*>(es);
    rn->grad = reinterpret_cast<float4*>(grad);
    rn->nbh = (int)((hidden_w_count(rn->net) / 4 + 63) / 64);
    rn->nbe = (int)((edge_count(rn->net) / 4 + 15) / 16);
    return true;
}

// the parameters of one network can be copied or mixed into the other's, images included
inline bool same_params(const MlpDev& a, const MlpDev& b) {
    return a.count == b.count && a.hp == b.hp && a.n_hidden == b.n_hidden;
}

// Adam's constants as the kernels take them (RedArgs, AdamArgs, AdamStep)
template <typename T>
void set_adam(T& a, float beta1, float beta2, float eps) {
    a.b1w = 1.0f - beta1;
    a.b2 = beta2;
    a.omb2 = 1.0f - beta2;
    a.eps = eps;
}

// The soft updates (robot.py:293-310) of n_pairs <= 4 (target, source) pairs as PolyArgs; the
// targets' images join *ps (nullable). False on the first pair that is no pair.
bool poly_pairs(const nav_mlp* targets, const nav_mlp* sources, int n_pairs, float tau,
                PackSet* ps, PolyArgs& a) {
    for (int i = 0; i < n_pairs; ++i) {
        MlpDev dt, ds;
        if (!make_dev(&targets[i], &dt) || !make_dev(&sources[i], &ds) || !same_params(dt, ds) ||
            (ps && !ps->add(&targets[i])))
            return false;
        a.q[i].t = reinterpret_cast<float4*>(targets[i].params);
        a.q[i].s = reinterpret_cast<const float4*>(sources[i].params);
        a.q[i].n4 = dt.count / 4;
        a.total4 += a.q[i].n4;
    }
    a.n = n_pairs;
    a.omt = 1.0f - tau;
    a.tau = tau;
    return true;
}
// the blocks a launch adds past its own for the pairs: one per kBlock float4, at most 256
inline int poly_blocks(const PolyArgs& a) {
    const int64_t b = (a.total4 + kBlock - 1) / kBlock;
    return a.n ? (int)(b < 256 ? b : 256) : 0;
}

// split count of a weight-gradient launch over n_groups networks (of every member) with M rows:
// WG_TOTAL workgroups (256: one 8-wave workgroup per CU) over all tile jobs, at least 512 rows
// per split
inline int32_t wgrad_splits(int64_t n_groups, int d_out, int hp, int n_hidden, int64_t M) {
    if (n_hidden < 2) return 1;
    int64_t s = WG_TOTAL / (n_groups * wgrad_tiling(d_out, hp, n_hidden).jobs);
    const int64_t by_rows = (M + 511) / 512;
    if (s > by_rows) s = by_rows;
    return (int32_t)(s < 1 ? 1 : s);
}

int wgrad_args(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* in, int32_t ld_in,
               int32_t in_col, const float* const* acts, const float* const* dz,
               const float* const* dy, int32_t ld_dy, const uint16_t* const* masks,
               float* const* slabs, int32_t splits, WgradArgs& a) {
    if (!nets || n_nets < 1 || n_nets > 2 || M < 1 || splits < 1 || !in || !dy || ld_dy < 0 ||
        !masks || !slabs)
        return NAV_EINVAL;
    for (int i = 0; i < n_nets; ++i) {
        if (!make_dev(&nets[i], &a.net[i]) || !dy[i] || !masks[i] || !slabs[i]) return NAV_EINVAL;
        if (a.net[i].hp != a.net[0].hp || a.net[i].d_in != a.net[0].d_in ||
            a.net[i].n_hidden != a.net[0].n_hidden || a.net[i].d_out != a.net[0].d_out)
            return NAV_EINVAL;
        a.acts[i] = acts ? acts[i] : nullptr;
        a.dz[i] = dz ? dz[i] : nullptr;
        if (a.net[i].n_hidden > 2 && (!a.acts[i] || !a.dz[i])) return NAV_EINVAL;
        a.dy[i] = dy[i];
        a.masks[i] = masks[i];
        a.slabs[i] = slabs[i];
    }
    if (in_col < 0 || in_col + a.net[0].d_in > ld_in) return NAV_EINVAL;
    a.M = M;
    a.in = in;
    a.ld_in = ld_in;
    a.in_col = in_col;
    a.ld_dy = ld_dy;
    a.splits = splits;
    const int hp = a.net[0].hp, nh = a.net[0].n_hidden;
    const WgradTiling tl = wgrad_tiling(a.net[0].d_out, hp, nh);
    a.tk = tl.tk;
    a.TT = tl.TT;
    a.tn = tl.tn;
    a.TN = tl.TN;
    a.n_hid = tl.jobs;
    // the factored path for the critics (d_out = 1); the actor's d_out = 2 would need two
    // accumulator sets and two splits per element (measured slower than wgrad_rows_mfma: 40 vs
    // 34 us at 2x256 on bf16, profiles/r04c; on the fp16 split 31.9 vs 25.4 us, r06r)
    a.fact = wgrad_fact_ok(hp, nh) && a.net[0].d_out == 1;
    // 32-row aligned splits and per-wave ranges: a chunk's mask row tiles start on a tile
    // boundary (at 64-row granularity a 100-row batch ran on 2 of the 8 waves: config 1's k_wgrad
    // 19.7 us, the generic path's rows loop ~30 k cycles, profiles/r06zf)
    a.per_split = ((M + splits - 1) / splits + 31) / 32 * 32;
    a.per_wave = ((a.per_split + WG_WAVES - 1) / WG_WAVES + 31) / 32 * 32;
    // whole 32-row tiles moved to the first wave of each SIMD pair, per 256 rows of a wave
    // (tools/wgrad_bench.py, profiles/r05ad_ab_wgrad_skew.txt: 0 / 32 / 64 / 96 rows for the
    // factored kernel -> 32.5 / 32.0 / 31.8 / 33.0 us, 0 / 64 / 96 / 128 for the operand path ->
    // 27.4 / 27.4 / 27.1 / 26.8 us; the 256 x 32 factored form re-tuned, r07c_ab_wgrad_skew.txt:
    // 0 / 32 / 64 / 96 -> 26.6 / 26.4 / 26.3 / 26.5 us, 64 kept)
    a.skew = (a.per_wave / 256) * (a.fact ? NAV_WG_SKEW_FACT : NAV_WG_SKEW_OPND);
    if ((int64_t)n_nets * a.n_hid * splits > ((int64_t)1 << 30)) return NAV_EINVAL;
    return 0;
}

// One weight-gradient launch from filled arguments: which of the entry point's five kernels
// k = {fact 256 x 32, fact 128 x 64, fact 64 x 64, gen, operand} runs, and its dynamic LDS
template <typename K, typename... A>
int wgrad_launch(const WgradArgs& a, K* const (&k)[5], dim3 grid, hipStream_t st, A... args) {
    // the factored kernel: its 4 KB fragment table is static, the dynamic part the reduce slots
    const size_t lds = a.fact ? (size_t)WG_WAVES * WG_TILE * WG_TILE * 4 : wgrad_lds_bytes();
    // >= 3 hidden layers: no tile is both the top and the first layer (no operand path)
    const int fact = a.tn == 256 ? 0 : a.tn == 128 ? 1 : 2;
    K* const f = k[a.fact ? fact : a.net[0].n_hidden >= 3 ? 3 : 4];
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(f),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(f, grid, dim3(WG_THREADS), lds, st, args...);
    NAV_CHECK_LAUNCH();
    return 0;
}

// RedArgs of the reduce (+ Adam when m is non-NULL, + the soft updates): *blocks = the reduce
// blocks of k_grad_reduce (a.red_blocks) plus its soft-update blocks
int red_args(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs, int32_t splits,
             const float* const* edge_slabs, int64_t edge_blocks, float* const* grads,
             float* const* m, float* const* v, float beta1, float beta2, float eps,
             const float* step_size, const float* bc2_sqrt, const nav_mlp* net_targets,
             const nav_mlp* targets, const nav_mlp* sources, int32_t n_pairs, float tau,
             RedArgs& a, int* blocks_out, PackSet* ps) {
    const bool adam = m != nullptr;
    if (!nets || n_nets < 1 || n_nets > 2 || !hidden_slabs || !edge_slabs || edge_blocks < 1 ||
        splits < 0 || (adam && (!v || !step_size || !bc2_sqrt)) || n_pairs < 0 || n_pairs > 4 ||
        (n_pairs && (!targets || !sources)) || (!adam && (n_pairs || net_targets || !grads)))
        return NAV_EINVAL;
    int blocks = 0;
    for (int i = 0; i < n_nets; ++i) {
        RedNet& rn = a.n[i];
        if (!edge_slabs[i] || (adam && (!m[i] || !v[i])) || (!adam && !grads[i]) ||
            !red_net(&nets[i], hidden_slabs[i], splits, edge_slabs[i], grads ? grads[i] : nullptr,
                     &rn))
            return NAV_EINVAL;
        if (rn.net.hp != a.n[0].net.hp || rn.net.n_hidden != a.n[0].net.n_hidden)
            return NAV_EINVAL;
        if (adam) {
            rn.p = reinterpret_cast<float4*>(nets[i].params);
            rn.m = reinterpret_cast<float4*>(m[i]);
            rn.v = reinterpret_cast<float4*>(v[i]);
            rn.step_size = step_size[i];
            rn.bc2s = bc2_sqrt[i];
            if (ps && !ps->add(&nets[i])) return NAV_EINVAL;
        }
        if (net_targets) {
            MlpDev dt;
            if (!make_dev(&net_targets[i], &dt) || !same_params(dt, rn.net)) return NAV_EINVAL;
            rn.tgt = reinterpret_cast<float4*>(net_targets[i].params);
            if (ps && !ps->add(&net_targets[i])) return NAV_EINVAL;
        }
        blocks += rn.nbh + rn.nbe;
    }
    if (!poly_pairs(targets, sources, n_pairs, tau, ps, a.poly)) return NAV_EINVAL;
    a.red_blocks = blocks;
    a.splits = splits;
    a.nblk = edge_blocks;
    set_adam(a, beta1, beta2, eps);
    *blocks_out = blocks + poly_blocks(a.poly);
    return 0;
}

}  // namespace
