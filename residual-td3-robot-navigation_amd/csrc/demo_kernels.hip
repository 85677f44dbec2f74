// demo_kernels.hip — the demonstrations' transitions as replay rows (nav_demo_transitions:
// process_demonstration's pushes, robot.py:704-716), in the learner's frame for the tail behind
// the replay ring and in the acting frame for the behaviour-cloning pretraining. A translation
// unit of its own: every other object of libnavenv.so compiles from the source it had before.
#include <stdlib.h>

#include "nav_device.h"

namespace {

using namespace nav;

// one thread per (demonstration d, step i < T-1): row d*(T-1)+i
__global__ __launch_bounds__(kBlock) void k_demo_transitions(
    nav_params p, int64_t n_rows, int32_t T, const float2* __restrict__ states,
    const float2* __restrict__ actions, const double2* __restrict__ goal, int32_t frame,
    float4* __restrict__ rows) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n_rows) return;
    const int64_t d = k / (T - 1);
    const int32_t i = (int32_t)(k - d * (T - 1));
    const float2 s = states[d * T + i], a = actions[d * T + i], ns = states[d * T + i + 1];
    const double2 g = goal[d];
    // compute_reward([s']) with no demonstration known yet (robot.py:741-750), the goal term as
    // the tick forms it (nav_tick.h)
    const double nx = (double)ns.x - g.x, ny = (double)ns.y - g.y;
    const double gt = -norm2(nx, ny);
    const double r = gt >= -p.goal_threshold ? p.goal_reward : gt;
    const float done = i == T - 2 ? 1.f : 0.f;
    float4 lo, hi;
    if (frame == 0) {
        lo = make_float4(s.x, s.y, a.x, a.y);
        hi = make_float4((float)r, ns.x, ns.y, done);
    } else {
        // the acting frame (robot.py:556, 586-588): the actor sees the baseline s - g and its
        // output is added to it, so the demonstrated, clipped action needs the residual
        // clamp(a) - (s - g); each value formed in double, rounded once
        const double sx = (double)s.x - g.x, sy = (double)s.y - g.y;
        const double m = p.max_action;
        const double cx = fmin(fmax((double)a.x, -m), m), cy = fmin(fmax((double)a.y, -m), m);
        lo = make_float4((float)sx, (float)sy, (float)(cx - sx), (float)(cy - sy));
        hi = make_float4((float)r, (float)nx, (float)ny, done);
    }
    rows[2 * k] = lo;
    rows[2 * k + 1] = hi;
}

}  // namespace

extern "C" int nav_demo_transitions(const nav_params* p, int32_t n_demo, int32_t T,
                                    const float* states, const float* actions, const double* goal,
                                    int32_t frame, float* rows, void* stream) {
    if (!p || !states || !actions || !goal || !rows || n_demo < 1 || T < 2 ||
        (frame != 0 && frame != 1))
        return NAV_EINVAL;
    const int64_t n_rows = (int64_t)n_demo * (T - 1);
    hipLaunchKernelGGL(k_demo_transitions, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, S(stream), *p, n_rows, T,
                       reinterpret_cast<const float2*>(states),
                       reinterpret_cast<const float2*>(actions),
                       reinterpret_cast<const double2*>(goal), frame,
                       reinterpret_cast<float4*>(rows));
    NAV_CHECK_LAUNCH();
    return 0;
}
