// Shared by the backward kernels of the cross_rows family (iqm_backward.hip, iqm_levels_backward.hip): the accumulator
// row map of v_mfma_f32_32x32x2_f32, the one chain every pass forms a probability with, the fixed reduction tree and the
// row-statistics kernel over the score / d_out-product records SG [B, keys, 32].
#pragma once
#include "common.h"
#include "kernels.h"

namespace aaclip {

// keys per slice of one image's (or one segment's) keys: a multiple of 64, at most CRB_MAX_SLICES slices
static inline int crb_per(int Lk) { return 64 * ((Lk + 64 * CRB_MAX_SLICES - 1) / (64 * CRB_MAX_SLICES)); }

namespace {

constexpr float CRB_LOG2E = 1.4426950408889634f;

AACLIP_DEV int crb_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }
AACLIP_DEV float crb_p(float s, float m, float linv) { return __builtin_amdgcn_exp2f((s - m) * CRB_LOG2E) * linv; }

template <typename T> AACLIP_DEV float crb_ld1(const T* p) { return (float)*p; }
template <typename T> AACLIP_DEV f32x4 crb_ld4(const T* p) {
  typedef T t4 __attribute__((ext_vector_type(4)));
  const t4 v = *(const t4*)p;
  return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

AACLIP_DEV float crb_block_sum(float v, float* red, int tid) {   // fixed tree over the 256 threads
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

}  // namespace

// grid (R, B): stats[(b * 16 + r) * 4 ..] = {max_j s, 1 / sum_j e^(s - max), delta}
static __global__ __launch_bounds__(256) void crb_stats_kernel(const float* __restrict__ sg, float* __restrict__ stats, int Lk) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const int q = blockIdx.x, b = blockIdx.y;
  const float* base = sg + (long)b * Lk * 32 + q;
  float m = -INFINITY;
  for (int j = tid; j < Lk; j += 256) m = fmaxf(m, base[(long)j * 32]);
  __syncthreads();
  red[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  float l = 0.f;
  for (int j = tid; j < Lk; j += 256) l += crb_p(base[(long)j * 32], m, 1.0f);
  l = crb_block_sum(l, red, tid);
  const float linv = 1.0f / l;
  float d = 0.f;
  for (int j = tid; j < Lk; j += 256) d = fmaf(crb_p(base[(long)j * 32], m, linv), base[(long)j * 32 + 16], d);
  d = crb_block_sum(d, red, tid);
  if (tid == 0) {
    float* o = stats + ((long)b * 16 + q) * 4;
    o[0] = m;
    o[1] = linv;
    o[2] = d;
  }
}

}  // namespace aaclip
