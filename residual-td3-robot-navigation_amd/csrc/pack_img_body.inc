// k_pack_img's statements on the PackArgs `a` (learner_kernels.hip includes this once per form)
    __shared__ float cmax[16][16];
    int b = blockIdx.x;
    const int jn = b / a.per_net;
    b -= jn * a.per_net;
    const PackJob& J = a.j[jn];
    const int hp = J.pk.hp;
    const int g = b % a.cg;
    b /= a.cg;
    const int which = b & 1, L = (b >> 1) + 1;
    if (L >= J.pk.n_hidden || g * 16 >= hp) return;  // workgroup-uniform
    const float* W = J.p + J.pk.w_off[L];
    float* img = J.pk.packed + (int64_t)(L - 1) * 2 * split_image_floats(hp) +
                 which * split_image_floats(hp);
    const int c = threadIdx.x & 15, kq = threadIdx.x >> 4;
    const int n = g * 16 + c, k0 = 16 * kq;
    const bool on = k0 < hp;  // hp is a multiple of 32 (and n < hp: whole 16-column groups)
    float v[16];
    float m = 0.f;
    if (on) {
        if (which == 0) {
            const float4* r = reinterpret_cast<const float4*>(W + (int64_t)n * hp + k0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 u = r[q];
                v[4 * q] = u.x; v[4 * q + 1] = u.y; v[4 * q + 2] = u.z; v[4 * q + 3] = u.w;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) v[t] = W[(int64_t)(k0 + t) * hp + n];
            if (J.pk.d_out == 1 && L == J.pk.n_hidden - 1) {  // workgroup-uniform
                const float* Wo = J.p + J.pk.w_off[J.pk.n_hidden];
#pragma unroll
                for (int t = 0; t < 16; ++t) v[t] = Wo[k0 + t] * v[t];
            }
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) m = fmaxf(m, fabsf(v[t]));
    }
    cmax[kq][c] = m;
    __syncthreads();
    if (!on) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) m = fmaxf(m, cmax[q][c]);
    const int e = pow2_exp(m);
    const float sc = ldexpf(1.f, e);
    _Float16* h16 = reinterpret_cast<_Float16*>(img);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        float xs[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) xs[t] = v[8 * half + t] * sc;
        const Split2 sp = split2_8(xs);
        const int k = k0 + 8 * half;
        *reinterpret_cast<f16x8*>(h16 + split_entry(hp, 0, k, n)) = sp.h;
        *reinterpret_cast<f16x8*>(h16 + split_entry(hp, 1, k, n)) = sp.l;
    }
    if (kq == 0) reinterpret_cast<int*>(img + (int64_t)hp * hp)[n] = e;
