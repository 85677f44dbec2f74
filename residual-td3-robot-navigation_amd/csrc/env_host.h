// env_host.h — what the entry points of env_kernels.hip, demo_reward.hip, demo_index.hip and
// demonstrator.hip share on the host (no kernel and no device code): the launch-and-check
// sequence, the HIP status mapping, the checks of an env set and a replay ring, the ring's slot
// origin, the DemoIdx builder and the casts of the C ABI's arrays to the kernels' vector types.
#pragma once
#include "nav_tick.h"

namespace {

using namespace nav;

// 0 or the negated HIP error
inline int hip_status(hipError_t e) { return e == hipSuccess ? 0 : -(int)e; }

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

// The arguments convert to the kernel's parameter types (P is deduced from the kernel alone).
template <typename T>
struct as_is { using type = T; };

// One launch without dynamic LDS, then the last error as the entry point's status.
template <typename... P>
inline int launch(void (*k)(P...), dim3 grid, dim3 block, void* stream,
                  typename as_is<P>::type... args) {
    hipLaunchKernelGGL(k, grid, block, 0, S(stream), args...);
    return hip_status(hipGetLastError());
}

// The one-lane-per-item kernels: kBlock lanes per workgroup over `items`.
template <typename... P>
inline int launch_items(void (*k)(P...), int64_t items, void* stream,
                        typename as_is<P>::type... args) {
    return launch(k, dim3(blocks_for(items)), dim3(kBlock), stream, args...);
}

inline bool env_ok(const nav_env_soa* e) {
    return e && e->n >= 0 && e->n < (int64_t)1 << 31 && (e->n == 0 || (e->state && e->goal &&
           e->region && e->hist && e->meta && e->plan_index && e->path_length && e->episodes &&
           e->noise_scale));
}

// A replay ring that rows can be pushed to from `base` on. slots: what one launch writes where it
// writes one slot per env (a ring smaller than that would let two envs write one slot).
inline bool ring_ok(const nav_replay* r, int64_t base, int64_t slots = 0) {
    return r && r->rows && r->capacity > 0 && r->capacity >= slots && base >= 0;
}
// the slot of a launch's item 0
inline int64_t ring_origin(const nav_replay* r, int64_t base) { return base % r->capacity; }

inline const double2* d2(const double* p) { return reinterpret_cast<const double2*>(p); }
inline double2* d2(double* p) { return reinterpret_cast<double2*>(p); }
inline const float2* f2(const float* p) { return reinterpret_cast<const float2*>(p); }
inline float2* f2(float* p) { return reinterpret_cast<float2*>(p); }
inline float4* f4(float* p) { return reinterpret_cast<float4*>(p); }

// shared demonstrations (no offsets) are one group: epg is not read, 1 keeps it a divisor
inline DemoIdx demo_idx(const double* demo_xy, const int64_t* demo_off, int32_t envs_per_group,
                        const int64_t* cell_start, const int32_t* cand) {
    return DemoIdx{d2(demo_xy), demo_off, envs_per_group > 0 ? envs_per_group : 1, cell_start,
                   cand};
}

}  // namespace
