// learner_kernels.hip — the cross-row half of the residual-TD3 learner (robot.py:236-310) on
// gfx950: hidden x hidden weight gradients on MFMA, the fixed-order gradient reduce fused with
// torch's Adam, multi-net Adam for the shared-policy bucket, Polyak soft updates (all refreshing
// the packed MFMA weight images), and the replay sampling / copy glue. The row-local half
// (forward, row backward, the fused train_critic / train_actor row programs) is rows_kernels.h
// and td3_rows.h.
// Here: the plain kernels and their C ABI. The device code they wrap is wgrad.h (weight
// gradients) and reduce_adam.h (reduce, Adam, Polyak), the argument checks and builders are
// learner_host.h; the population forms of the same bodies are learner_pop.hip.
#include "learner_host.h"

namespace {

// grid: nets x tile jobs x splits workgroups of 8 waves (one kernel per path: each gets its own
// register allocation)
__global__ __launch_bounds__(WG_THREADS) void k_wgrad(WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    wgrad_tile<false>(a, wgrad_job(a, blockIdx.x, gridDim.x), smem);
}
__global__ __launch_bounds__(WG_THREADS) void k_wgrad_gen(WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    wgrad_tile<true>(a, wgrad_job(a, blockIdx.x, gridDim.x), smem);
}
template <int NI, int D, int KH>
__global__ __launch_bounds__(WG_THREADS) void k_wgrad_fact(WgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ uint4 tab[256];
    wgrad_tile_fact<NI, D, KH>(a, wgrad_job(a, blockIdx.x, gridDim.x), smem, tab);
}

// (the statements are pack_img_body.inc, once per form: the plain kernel's machine code is
// pinned, and reaching `a` through a shared device function changed its register allocation)
__global__ __launch_bounds__(kBlock) void k_pack_img(PackArgs a) {
#include "pack_img_body.inc"
}

template <bool ADAM>
__global__ __launch_bounds__(kBlock) void k_grad_reduce(RedArgs a) {
    grad_reduce_body<ADAM, false>(a, AdamStep{});
}

__global__ __launch_bounds__(kBlock) void k_adam(float4* __restrict__ p,
                                                 const float4* __restrict__ g, float4* m,
                                                 float4* v, int64_t n4, float b1w, float b2,
                                                 float omb2, float eps, float ss, float bc2s) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * kBlock) {
        float4 pp = p[i], gg = g[i], mm = m[i], vv = v[i];
        adam1(pp.x, gg.x, mm.x, vv.x, b1w, b2, omb2, eps, ss, bc2s);
        adam1(pp.y, gg.y, mm.y, vv.y, b1w, b2, omb2, eps, ss, bc2s);
        adam1(pp.z, gg.z, mm.z, vv.z, b1w, b2, omb2, eps, ss, bc2s);
        adam1(pp.w, gg.w, mm.w, vv.w, b1w, b2, omb2, eps, ss, bc2s);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// torch.optim.Adam of up to 2 networks in one launch from flat gradients that a collective
// produced (shared policy: the SUM all-reduce of the bucket); g / grad_div is the averaged
// gradient (grad_div 1: the plain step, bit-identical to k_adam). With the soft updates (a
// policy epoch, nav_adam_polyak_multi): each net's own target follows its stepped parameters
// (k_polyak's expression, as in the fused reduce), and the extra (target, source) pairs run on
// the blocks past the Adam blocks — the hook path's counterpart of nav_grad_reduce_adam_polyak.
__global__ __launch_bounds__(kBlock) void k_adam_multi(AdamArgs a) {
    if ((int)blockIdx.x >= a.adam_blocks) {  // the extra soft-update pairs (block-uniform)
        for (int64_t i = (int64_t)(blockIdx.x - a.adam_blocks) * kBlock + threadIdx.x;
             i < a.poly.total4; i += (int64_t)(gridDim.x - a.adam_blocks) * kBlock)
            polyak_elem(a.poly, i);
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.total4;
         i += (int64_t)a.adam_blocks * kBlock) {
        const bool second = a.n > 1 && i >= a.q[0].n4;
        const AdamNet& q = second ? a.q[1] : a.q[0];
        const int64_t j = second ? i - a.q[0].n4 : i;
        float4 pp = q.p[j], gg = q.g[j], mm = q.m[j], vv = q.v[j];
        gg.x = gg.x / a.gdiv; gg.y = gg.y / a.gdiv; gg.z = gg.z / a.gdiv; gg.w = gg.w / a.gdiv;
        adam1(pp.x, gg.x, mm.x, vv.x, a.b1w, a.b2, a.omb2, a.eps, q.step_size, q.bc2s);
        adam1(pp.y, gg.y, mm.y, vv.y, a.b1w, a.b2, a.omb2, a.eps, q.step_size, q.bc2s);
        adam1(pp.z, gg.z, mm.z, vv.z, a.b1w, a.b2, a.omb2, a.eps, q.step_size, q.bc2s);
        adam1(pp.w, gg.w, mm.w, vv.w, a.b1w, a.b2, a.omb2, a.eps, q.step_size, q.bc2s);
        q.p[j] = pp; q.m[j] = mm; q.v[j] = vv;
        if (q.tgt) {  // robot.py:309 on the parameter just stepped
            float4 t = q.tgt[j];
            t.x = t.x * a.poly.omt + pp.x * a.poly.tau;
            t.y = t.y * a.poly.omt + pp.y * a.poly.tau;
            t.z = t.z * a.poly.omt + pp.z * a.poly.tau;
            t.w = t.w * a.poly.omt + pp.w * a.poly.tau;
            q.tgt[j] = t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_polyak(float4* __restrict__ t,
                                                   const float4* __restrict__ s, int64_t n4,
                                                   float omt, float tau) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * kBlock) {
        float4 a = t[i];
        const float4 b = s[i];
        // robot.py:309 target*(1-tau) + source*tau (two products, one sum)
        a.x = a.x * omt + b.x * tau;
        a.y = a.y * omt + b.y * tau;
        a.z = a.z * omt + b.z * tau;
        a.w = a.w * omt + b.w * tau;
        t[i] = a;
    }
}

__global__ __launch_bounds__(kBlock) void k_polyak_multi(PolyArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.total4;
         i += (int64_t)gridDim.x * kBlock)
        polyak_elem(a, i);
}

// ---------------- TD3 glue ----------------
__global__ __launch_bounds__(kBlock) void k_replay_sample(const float4* __restrict__ rows,
                                                          int64_t size, int64_t B,
                                                          const int64_t* __restrict__ idx,
                                                          uint32_t s0, uint32_t s1, uint32_t ctr,
                                                          float4* __restrict__ batch) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    int64_t k;
    if (idx) {
        k = idx[b];
    } else {
        const uint4 w = philox((uint32_t)b, 0u, NAV_TAG_SAMPLE, ctr, s0, s1);
        k = (int64_t)(((uint64_t)w.x * (uint64_t)size) >> 32);
    }
    batch[2 * b] = rows[2 * k];
    batch[2 * b + 1] = rows[2 * k + 1];
}

// One epoch's sample indices with demonstration rows mixed in (nav_td3_mix_idx): out[0] at Philox
// counter ctr0 (the critic's batch), out[1] at ctr0 + 1 (the actor's); rows b < B_demo from
// NAV_TAG_DEMO over the n_demo rows at demo_base, the rest what sample_row draws itself
struct MixIdxArgs {
    int64_t size, B, B_demo, demo_base, n_demo;
    uint32_t s0, s1, ctr0;
    int64_t* out[2];
};
__global__ __launch_bounds__(kBlock) void k_td3_mix_idx(MixIdxArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= a.B) return;
    const bool demo = b < a.B_demo;
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        if (!a.out[y]) continue;
        const uint4 w = philox((uint32_t)b, 0u, demo ? NAV_TAG_DEMO : NAV_TAG_SAMPLE,
                               a.ctr0 + (uint32_t)y, a.s0, a.s1);
        a.out[y][b] = demo ? a.demo_base + (int64_t)(((uint64_t)w.x * (uint64_t)a.n_demo) >> 32)
                           : (int64_t)(((uint64_t)w.x * (uint64_t)a.size) >> 32);
    }
}

__global__ __launch_bounds__(kBlock) void k_fill(float* x, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) x[i] = v;
}

__global__ __launch_bounds__(kBlock) void k_strided_copy(const float* __restrict__ src, int lds,
                                                         int cs, float* __restrict__ dst, int ldd,
                                                         int cd, int64_t rows, int cols) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t r = i / cols;
    const int c = (int)(i % cols);
    dst[r * ldd + cd + c] = src[r * lds + cs + c];
}

// the images of the set's networks, rebuilt on the writer's stream
int pack_launch(PackSet& ps, hipStream_t st) {
    PackArgs& a = ps.a;
    if (a.n == 0) return 0;
    ps.shape();
    hipLaunchKernelGGL(k_pack_img, dim3((unsigned)(a.n * a.per_net)), dim3(kBlock), 0, st, a);
    NAV_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int32_t nav_mlp_wgrad_splits(int32_t n_nets, int32_t d_out, int32_t hidden_pad, int32_t n_hidden,
                             int64_t M) {
    if (n_nets < 1 || n_nets > 2 || d_out < 1 || d_out > 2 || hidden_pad < 32 ||
        hidden_pad > 256 || (hidden_pad & 31) || n_hidden < 1 || M < 0)
        return NAV_EINVAL;
    return wgrad_splits(n_nets, d_out, hidden_pad, n_hidden, M);
}

int nav_mlp_wgrad(const nav_mlp* nets, int32_t n_nets, int64_t M, const float* in,
                  int32_t ld_in, int32_t in_col, const float* const* acts,
                  const float* const* dz, const float* const* dy, int32_t ld_dy,
                  const uint16_t* const* masks, float* const* slabs, int32_t splits,
                  void* stream) {
    WgradArgs a{};
    const int rc = wgrad_args(nets, n_nets, M, in, ld_in, in_col, acts, dz, dy, ld_dy, masks,
                              slabs, splits, a);
    if (rc) return rc;
    if (a.net[0].n_hidden < 2) return 0;
    const int64_t blocks = (int64_t)n_nets * a.n_hid * splits;
    void (*const k[5])(WgradArgs) = {k_wgrad_fact<8, 1, 1>, k_wgrad_fact<4, 1, 2>,
                                     k_wgrad_fact<2, 1, 2>, k_wgrad_gen, k_wgrad};
    return wgrad_launch(a, k, dim3((unsigned)blocks), S(stream), a);
}

int nav_grad_reduce_multi(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs,
                          int32_t splits, const float* const* edge_slabs, int64_t edge_blocks,
                          float* const* grads, void* stream) {
    RedArgs a{};
    int blocks = 0;
    const int rc = red_args(nets, n_nets, hidden_slabs, splits, edge_slabs, edge_blocks, grads,
                            nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr,
                            nullptr, 0, 0.f, a, &blocks, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_grad_reduce<false>, dim3((unsigned)blocks), dim3(kBlock), 0, S(stream),
                       a);
    NAV_CHECK_LAUNCH();
    return 0;
}

// the one-network case (hidden_slabs may be NULL for a 1-hidden-layer network, which has none)
int nav_grad_reduce(const nav_mlp* net, const float* hidden_slabs, int32_t splits,
                    const float* edge_slabs, int64_t edge_blocks, float* grad, void* stream) {
    return nav_grad_reduce_multi(net, 1, &hidden_slabs, splits, &edge_slabs, edge_blocks, &grad,
                                 stream);
}

static int adam_multi_impl(const nav_mlp* nets, int32_t n_nets, const float* const* grads,
                           float* const* m, float* const* v, float beta1, float beta2, float eps,
                           const float* step_size, const float* bc2_sqrt, float grad_div,
                           const nav_mlp* net_targets, const nav_mlp* targets,
                           const nav_mlp* sources, int32_t n_pairs, float tau, void* stream) {
    AdamArgs a{};
    PackSet ps;
    if (!nets || n_nets < 1 || n_nets > 2 || !grads || !m || !v || !step_size || !bc2_sqrt ||
        !(grad_div > 0.f) || n_pairs < 0 || n_pairs > 4 || (n_pairs && (!targets || !sources)))
        return NAV_EINVAL;
    for (int i = 0; i < n_nets; ++i) {
        MlpDev d;
        if (!make_dev(&nets[i], &d) || !grads[i] || !m[i] || !v[i]) return NAV_EINVAL;
        AdamNet& q = a.q[i];
        q.p = reinterpret_cast<float4*>(nets[i].params);
        q.g = reinterpret_cast<const float4*>(grads[i]);
        q.m = reinterpret_cast<float4*>(m[i]);
        q.v = reinterpret_cast<float4*>(v[i]);
        q.n4 = d.count / 4;
        q.step_size = step_size[i];
        q.bc2s = bc2_sqrt[i];
        if (!ps.add(&nets[i])) return NAV_EINVAL;
        if (net_targets) {
            MlpDev dt;
            if (!make_dev(&net_targets[i], &dt) || !same_params(dt, d) ||
                !ps.add(&net_targets[i]))
                return NAV_EINVAL;
            q.tgt = reinterpret_cast<float4*>(net_targets[i].params);
        }
        a.total4 += q.n4;
    }
    if (!poly_pairs(targets, sources, n_pairs, tau, &ps, a.poly)) return NAV_EINVAL;
    a.n = n_nets;
    set_adam(a, beta1, beta2, eps);
    a.gdiv = grad_div;
    a.adam_blocks = grid_stride_blocks(a.total4);
    const int blocks = a.adam_blocks + poly_blocks(a.poly);
    hipLaunchKernelGGL(k_adam_multi, dim3((unsigned)blocks), dim3(kBlock), 0, S(stream), a);
    NAV_CHECK_LAUNCH();
    return pack_launch(ps, S(stream));
}

int nav_adam_multi(const nav_mlp* nets, int32_t n_nets, const float* const* grads,
                   float* const* m, float* const* v, float beta1, float beta2, float eps,
                   const float* step_size, const float* bc2_sqrt, float grad_div, void* stream) {
    return adam_multi_impl(nets, n_nets, grads, m, v, beta1, beta2, eps, step_size, bc2_sqrt,
                           grad_div, nullptr, nullptr, nullptr, 0, 0.f, stream);
}

int nav_adam_polyak_multi(const nav_mlp* nets, int32_t n_nets, const float* const* grads,
                          float* const* m, float* const* v, float beta1, float beta2, float eps,
                          const float* step_size, const float* bc2_sqrt, float grad_div,
                          const nav_mlp* net_targets, const nav_mlp* targets,
                          const nav_mlp* sources, int32_t n_pairs, float tau, void* stream) {
    if (!net_targets) return NAV_EINVAL;
    return adam_multi_impl(nets, n_nets, grads, m, v, beta1, beta2, eps, step_size, bc2_sqrt,
                           grad_div, net_targets, targets, sources, n_pairs, tau, stream);
}

static int grad_reduce_adam_impl(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs,
                          int32_t splits, const float* const* edge_slabs, int64_t edge_blocks,
                          float* const* grads, float* const* m, float* const* v, float beta1,
                          float beta2, float eps, const float* step_size, const float* bc2_sqrt,
                          const nav_mlp* net_targets, const nav_mlp* targets,
                          const nav_mlp* sources, int32_t n_pairs, float tau, void* stream) {
    RedArgs a{};
    PackSet ps;
    int blocks = 0;
    if (!m) return NAV_EINVAL;
    const int rc = red_args(nets, n_nets, hidden_slabs, splits, edge_slabs, edge_blocks, grads, m,
                            v, beta1, beta2, eps, step_size, bc2_sqrt, net_targets, targets,
                            sources, n_pairs, tau, a, &blocks, &ps);
    if (rc) return rc;
    hipLaunchKernelGGL(k_grad_reduce<true>, dim3((unsigned)blocks), dim3(kBlock), 0, S(stream),
                       a);
    NAV_CHECK_LAUNCH();
    return pack_launch(ps, S(stream));
}

int nav_grad_reduce_adam(const nav_mlp* nets, int32_t n_nets, const float* const* hidden_slabs,
                         int32_t splits, const float* const* edge_slabs, int64_t edge_blocks,
                         float* const* grads, float* const* m, float* const* v, float beta1,
                         float beta2, float eps, const float* step_size, const float* bc2_sqrt,
                         void* stream) {
    return grad_reduce_adam_impl(nets, n_nets, hidden_slabs, splits, edge_slabs, edge_blocks,
                                 grads, m, v, beta1, beta2, eps, step_size, bc2_sqrt, nullptr,
                                 nullptr, nullptr, 0, 0.f, stream);
}

int nav_grad_reduce_adam_polyak(const nav_mlp* nets, int32_t n_nets,
                                const float* const* hidden_slabs, int32_t splits,
                                const float* const* edge_slabs, int64_t edge_blocks,
                                float* const* grads, float* const* m, float* const* v,
                                float beta1, float beta2, float eps, const float* step_size,
                                const float* bc2_sqrt, const nav_mlp* net_targets,
                                const nav_mlp* targets, const nav_mlp* sources, int32_t n_pairs,
                                float tau, void* stream) {
    if (!net_targets) return NAV_EINVAL;
    return grad_reduce_adam_impl(nets, n_nets, hidden_slabs, splits, edge_slabs, edge_blocks,
                                 grads, m, v, beta1, beta2, eps, step_size, bc2_sqrt, net_targets,
                                 targets, sources, n_pairs, tau, stream);
}

int nav_polyak_multi(const nav_mlp* targets, const nav_mlp* sources, int32_t n, float tau,
                     void* stream) {
    PolyArgs a{};
    PackSet ps;
    if (!targets || !sources || n < 1 || n > 4 || !poly_pairs(targets, sources, n, tau, &ps, a))
        return NAV_EINVAL;
    hipLaunchKernelGGL(k_polyak_multi, dim3(grid_stride_blocks(a.total4)), dim3(kBlock), 0,
                       S(stream), a);
    NAV_CHECK_LAUNCH();
    return pack_launch(ps, S(stream));
}

int nav_adam(const nav_mlp* net, const float* grad, float* m, float* v, float beta1, float beta2,
             float eps, float step_size, float bc2_sqrt, void* stream) {
    MlpDev d;
    if (!make_dev(net, &d) || !grad || !m || !v) return NAV_EINVAL;
    const int64_t n4 = d.count / 4;
    hipLaunchKernelGGL(k_adam, dim3(grid_stride_blocks(n4)), dim3(kBlock), 0, S(stream),
                       reinterpret_cast<float4*>(net->params),
                       reinterpret_cast<const float4*>(grad), reinterpret_cast<float4*>(m),
                       reinterpret_cast<float4*>(v), n4, 1.0f - beta1, beta2, 1.0f - beta2, eps,
                       step_size, bc2_sqrt);
    NAV_CHECK_LAUNCH();
    PackSet ps;
    ps.add(net);
    return pack_launch(ps, S(stream));
}

int nav_polyak(const nav_mlp* target, const nav_mlp* source, float tau, void* stream) {
    MlpDev dt, ds;
    if (!make_dev(target, &dt) || !make_dev(source, &ds) || !same_params(dt, ds))
        return NAV_EINVAL;
    const int64_t n4 = dt.count / 4;
    hipLaunchKernelGGL(k_polyak, dim3(grid_stride_blocks(n4)), dim3(kBlock), 0, S(stream),
                       reinterpret_cast<float4*>(target->params),
                       reinterpret_cast<const float4*>(source->params), n4, 1.0f - tau, tau);
    NAV_CHECK_LAUNCH();
    PackSet ps;
    ps.add(target);
    return pack_launch(ps, S(stream));
}

int nav_mlp_pack(const nav_mlp* net, void* stream) {
    MlpDev d;
    if (!make_dev(net, &d)) return NAV_EINVAL;
    if (d.n_hidden < 2) return 0;
    if (!net->packed) return NAV_EINVAL;
    PackSet ps;
    ps.add(net);
    return pack_launch(ps, S(stream));
}

int nav_replay_sample(const nav_replay* replay, int64_t size, int64_t B, const int64_t* idx,
                      uint32_t seed_lo, uint32_t seed_hi, uint32_t counter, float* batch,
                      void* stream) {
    if (!replay || !replay->rows || size < 1 || size > replay->capacity ||
        size > ((int64_t)1 << 32) || B < 0 || !batch)
        return NAV_EINVAL;
    if (B == 0) return 0;
    hipLaunchKernelGGL(k_replay_sample, dim3(blocks_for(B)), dim3(kBlock), 0, S(stream),
                       reinterpret_cast<const float4*>(replay->rows), size, B, idx, seed_lo,
                       seed_hi, counter, reinterpret_cast<float4*>(batch));
    NAV_CHECK_LAUNCH();
    return 0;
}

int nav_td3_mix_idx(int64_t size, int64_t B, int64_t B_demo, int64_t demo_base, int64_t n_demo,
                    uint32_t seed_lo, uint32_t seed_hi, uint32_t counter, int64_t* idx_critic,
                    int64_t* idx_actor, void* stream) {
    if (B < 1 || size < 1 || size > ((int64_t)1 << 32) || B_demo < 0 || B_demo > B ||
        (B_demo > 0 && (n_demo < 1 || n_demo > ((int64_t)1 << 32))) || demo_base < 0)
        return NAV_EINVAL;
    if (!idx_critic && !idx_actor) return 0;
    MixIdxArgs a{size, B, B_demo, demo_base, n_demo, seed_lo, seed_hi, 2u * counter,
                 {idx_critic, idx_actor}};
    hipLaunchKernelGGL(k_td3_mix_idx, dim3(blocks_for(B)), dim3(kBlock), 0, S(stream), a);
    NAV_CHECK_LAUNCH();
    return 0;
}

int nav_fill(float* x, int64_t n, float value, void* stream) {
    if (n < 0 || (n && !x)) return NAV_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_fill, dim3(blocks_for(n)), dim3(kBlock), 0, S(stream), x, n, value);
    NAV_CHECK_LAUNCH();
    return 0;
}

int nav_strided_copy(const float* src, int32_t ld_src, int32_t col_src, float* dst,
                     int32_t ld_dst, int32_t col_dst, int64_t rows, int32_t cols, void* stream) {
    if (rows < 0 || cols < 0 || (rows && cols && (!src || !dst))) return NAV_EINVAL;
    if (rows == 0 || cols == 0) return 0;
    hipLaunchKernelGGL(k_strided_copy, dim3(blocks_for(rows * cols)), dim3(kBlock), 0, S(stream),
                       src, ld_src, col_src, dst, ld_dst, col_dst, rows, cols);
    NAV_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

#ifdef NAV_WGRAD_TRACE
extern "C" int nav_wgrad_trace_read(unsigned long long* host, int n) {
    const size_t bytes = sizeof(g_wgrad_trace);
    if (!host || (size_t)n * sizeof(unsigned long long) < bytes) return NAV_EINVAL;
    const hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wgrad_trace), bytes);
    return e == hipSuccess ? 0 : -(int)e;
}
#endif
