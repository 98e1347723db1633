// The device code of the LARS step, shared by mae_lars_step (k_probe.hip: one segment, blocks on x) and mae_lars_step_groups
// (k_probe_sweep.hip: the same per group, the group on blockIdx.y).  One copy of every expression, so a group gets the bits the
// single call gives on that segment alone.  `bx` / `nbx` are the block's index and the block count along x.
#pragma once
#include "common.cuh"

namespace mae {

constexpr int LARS_BLOCKS = 1024;                           // stage-1 partials per norm
constexpr int LARS_SCRATCH_FLOATS = 4096;  // per segment: 2 * LARS_BLOCKS partials, then |p|, |dp|, q

inline int lars_sum_grid(int64_t n4) { return (int)std::min<int64_t>(cdiv(n4, 256), LARS_BLOCKS); }
inline int lars_update_grid(int64_t n4) { return (int)std::min<int64_t>(cdiv(n4, 256), 256 * 16); }

__device__ __forceinline__ void lars_sumsq_block(const float* __restrict__ p, const float* __restrict__ g, int64_t n4, float wd,
                                                 float* __restrict__ partial, unsigned bx, unsigned nbx) {
  __shared__ float red[4];
  float ap = 0.f, au = 0.f;
  for (int64_t i = bx * 256ll + threadIdx.x; i < n4; i += (int64_t)nbx * 256) {
    const f32x4 v = load4(p + i * 4);
    const f32x4 d = load4(g + i * 4) + v * wd;
    ap += sumsq4(v);
    au += sumsq4(d);
  }
  ap = block_sum_256(ap, red);
  au = block_sum_256(au, red);
  if (threadIdx.x == 0) {
    partial[bx] = ap;
    partial[LARS_BLOCKS + bx] = au;
  }
}

// stats[0] = |p|, stats[1] = |dp|, stats[2] = q
__device__ __forceinline__ void lars_finalize_block(const float* __restrict__ partial, int nb, float trust, float* __restrict__ stats,
                                                    float* __restrict__ norms_out) {
  __shared__ float red[4];
  float ap = 0.f, au = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) {
    ap += partial[i];
    au += partial[LARS_BLOCKS + i];
  }
  ap = block_sum_256(ap, red);
  au = block_sum_256(au, red);
  if (threadIdx.x == 0) {
    const float pn = sqrtf(ap), un = sqrtf(au);
    stats[0] = pn;
    stats[1] = un;
    stats[2] = (pn > 0.f && un > 0.f) ? trust * pn / un : 1.0f;
    if (norms_out) {
      norms_out[0] = pn;
      norms_out[1] = un;
    }
  }
}

template <bool ADAPT>
__device__ __forceinline__ void lars_update_block(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu, int64_t n4,
                                                  float lr, float momentum, float wd, const float* __restrict__ stats, unsigned bx, unsigned nbx) {
  const float q = ADAPT ? stats[2] : 1.0f;
  for (int64_t i = bx * 256ll + threadIdx.x; i < n4; i += (int64_t)nbx * 256) {
    f32x4 pp = load4(p + i * 4);
    f32x4 d = load4(g + i * 4);
    if (ADAPT) d = (d + pp * wd) * q;
    const f32x4 m = load4(mu + i * 4) * momentum + d;
    pp -= m * lr;
    store4(mu + i * 4, m);
    store4(p + i * 4, pp);
  }
}

}  // namespace mae
