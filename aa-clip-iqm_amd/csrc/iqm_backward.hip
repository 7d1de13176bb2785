// Backward of aaclip_cross_rows (iqm.hip): per image b, R effective queries qt[b, r] over the raw rows x[b, j], j < Lk:
//   s_rj = qt_r . x_j,  p_r = softmax_j s_r,  out_r = sum_j p_rj x_j
// and from d_out [B, R, Dk], with g_rj = d_out_r . x_j and delta_r = sum_j p_rj g_rj:
//   ds_rj = p_rj (g_rj - delta_r),  d_qt_r = sum_j ds_rj x_j,  d_x_j = sum_r (p_rj d_out_r + ds_rj qt_r).
// Nothing of size Lk x Dk is kept: the scores are recomputed.  All products run on v_mfma_f32_32x32x2_f32 (an exact
// fmaf chain; operand maps in attention_backward.hip: lane = 32 h + r holds A[row r][k = h] and B[k = h][col r],
// accumulator element e = D[row (e & 3) + 8 (e >> 2) + 4 h][col r]).  The keys of an image are cut into slices of
// `per` keys (a multiple of 64, at most CRB_MAX_SLICES slices); a workgroup of four waves owns a slice and walks it in
// tiles of 32 keys, and wave w owns the columns [w Dk / 4, (w + 1) Dk / 4) of every row, so that the query-side
// operands of a wave (32 x Dk / 4 values) stay in registers for the whole slice.
//   crb_scores_kernel   SG[b, j, 0:16] = s_.j and SG[b, j, 16:32] = g_.j as ONE [32 keys x Dk] . [Dk x 32] product per
//                       tile ([qt ; d_out] padded to 16 + 16 columns); each wave sums its quarter of Dk, the four
//                       quarters are added in wave order through LDS.
//   crb_stats_kernel    (crb_common.h) per (b, r): m = max_j s, 1 / sum_j e^(s - m) and delta_r = sum_j p_rj g_rj,
//                       read from SG.  One
//                       workgroup per row reduces over all keys with a fixed tree, so there are no per-slice (m, l)
//                       partials to merge: SG is Lk x 32 floats per image and stays in L2.  delta comes from the very
//                       p g products it is subtracted from, not from a forward output.
//   crb_grad_kernel     per tile: p and ds from SG and the statistics (crb_p: the one chain every pass forms a
//                       probability with); d_x tile = [P | dS] [32 x 32] . [d_out ; qt] [32 x Dk / 4 per wave], with the
//                       activation slope and `accumulate` applied at the store; dS^T X [16 x Dk / 4] accumulates in
//                       registers over the slice's tiles and is written as the slice's partial of d_qt.
//   crb_combine_kernel  d_qt = the slices' partials added in slice order.
// No atomics; every output element is written by one thread and summed in a fixed order: two calls give the same bits.
#include "common.h"
#include "crb_common.h"
#include "kernels.h"

namespace aaclip {

// grid (slices, B).  Column c of the right-hand side: qt row c for c < 16, d_out row c - 16 otherwise (zero past R).
// The k index of MFMA step 4 c + e in half h is column d0 + 8 c + 4 h + e of the rows: both halves load 16 bytes.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void crb_scores_kernel(const float* __restrict__ qt, const float* __restrict__ dout,
                                                         const T* __restrict__ x, float* __restrict__ sg, int R, int Lk,
                                                         int per) {
  constexpr int Dk = NCH * 256, DW = NCH * 64;
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y;
  const int j0 = blockIdx.x * per, j1 = min(Lk, j0 + per);
  const int d0 = wave * DW;
  float qd[DW / 2];
  {
    const int q = r & 15;
    const float* src = (r < 16 ? qt : dout) + ((long)b * R + (q < R ? q : 0)) * Dk + d0 + 4 * h;
#pragma unroll
    for (int c = 0; c < DW / 8; ++c) {
      const f32x4 v = *(const f32x4*)(src + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) qd[4 * c + e] = q < R ? v[e] : 0.f;
    }
  }
  for (int t0 = j0; t0 < j1; t0 += 32) {
    int row = t0 + r;
    row = row < j1 ? row : j1 - 1;
    const T* xr = x + ((long)b * Lk + row) * Dk + d0 + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < DW / 8; ++c) {
      const f32x4 v = crb_ld4(xr + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e], qd[4 * c + e], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][e][lane] = acc[e];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = tid + 256 * k;
      const int e = idx >> 6, ln = idx & 63;
      const float v = ((red[0][e][ln] + red[1][e][ln]) + red[2][e][ln]) + red[3][e][ln];
      const int key = t0 + crb_row(e, ln >> 5);
      if (key < j1) sg[((long)b * Lk + key) * 32 + (ln & 31)] = v;
    }
    __syncthreads();
  }
}

// grid (slices, B).  d_x or part may be null (not both).  neg = the activation's slope for x <= 0 (1 without one).
template <typename T, int NCH>
__global__ __launch_bounds__(256) void crb_grad_kernel(const float* __restrict__ qt, const float* __restrict__ dout,
                                                       const T* __restrict__ x, const float* __restrict__ sg,
                                                       const float* __restrict__ stats, float* __restrict__ d_x,
                                                       float* __restrict__ part, int R, int Lk, int per, int act,
                                                       float neg, int accumulate) {
  constexpr int Dk = NCH * 256, DW = NCH * 64, NB = DW / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, sl = blockIdx.x;
  const int j0 = sl * per, j1 = min(Lk, j0 + per);
  const int d0 = wave * DW;
  const float* st = stats + (long)b * 16 * 4;
  const long xb = (long)b * Lk;

  // d_x: step i of the [P | dS] . [d_out ; qt] product is row c = 2 i + h: d_out row c for i < 8, qt row c - 16 after
  float dq[NB][16];
  float m8[8], li8[8], de8[8];
  if (d_x) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = 2 * (i & 7) + h;
      const float* src = (i < 8 ? dout : qt) + ((long)b * R + (q < R ? q : 0)) * Dk + d0 + r;
#pragma unroll
      for (int k = 0; k < NB; ++k) dq[k][i] = q < R ? src[32 * k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q = 2 * i + h;
      const bool on = q < R;
      m8[i] = on ? st[q * 4] : 0.f;
      li8[i] = on ? st[q * 4 + 1] : 0.f;
      de8[i] = on ? st[q * 4 + 2] : 0.f;
    }
  }
  // d_qt: row r of dS^T (r < R), the statistics of query r
  const bool qrow = r < R;   // R <= 16
  const float m2 = qrow ? st[r * 4] : 0.f, li2 = qrow ? st[r * 4 + 1] : 0.f, de2 = qrow ? st[r * 4 + 2] : 0.f;
  f32x16 aq[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k)
#pragma unroll
    for (int e = 0; e < 16; ++e) aq[k][e] = 0.f;

  for (int t0 = j0; t0 < j1; t0 += 32) {
    if (d_x) {
      const bool alive = t0 + r < j1;
      const float* sr = sg + (xb + (alive ? t0 + r : j1 - 1)) * 32;
      f32x4 sv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) sv[c] = *(const f32x4*)(sr + 4 * c);
      float a[16];
#pragma unroll
      for (int i = 0; i < 8; ++i) {   // query 2 i + h: element 2 (i & 1) + h of chunk i / 2 (s) and 4 + i / 2 (g)
        const float s = h ? sv[i >> 1][2 * (i & 1) + 1] : sv[i >> 1][2 * (i & 1)];
        const float g = h ? sv[4 + (i >> 1)][2 * (i & 1) + 1] : sv[4 + (i >> 1)][2 * (i & 1)];
        const float p = (alive && 2 * i + h < R) ? crb_p(s, m8[i], li8[i]) : 0.f;
        a[i] = p;
        a[8 + i] = p * (g - de8[i]);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], dq[k][i], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = t0 + crb_row(e, h);
          if (key < j1) {
            const long o = (xb + key) * Dk + d0 + 32 * k + r;
            float v = acc[e];
            if (act) v *= crb_ld1(x + o) > 0.f ? 1.0f : neg;
            if (accumulate) v = d_x[o] + v;
            d_x[o] = v;
          }
        }
      }
    }
    if (part) {
      float a2[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = t0 + 2 * i + h;
        const bool alive = key < j1 && qrow;
        const float* sr = sg + (xb + (key < j1 ? key : j1 - 1)) * 32 + (r & 15);
        const float p = alive ? crb_p(sr[0], m2, li2) : 0.f;
        a2[i] = p * (sr[16] - de2);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = t0 + 2 * i + h;
          const float xv = crb_ld1(x + (xb + (key < j1 ? key : j1 - 1)) * Dk + d0 + 32 * k + r);
          aq[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[i], xv, aq[k], 0, 0, 0);
        }
    }
  }
  if (part) {
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // accumulator rows 0 .. 15 are elements 0 .. 7 of both halves
        const int q = crb_row(e, h);
        if (q < R) part[(((long)b * gridDim.x + sl) * R + q) * Dk + d0 + 32 * k + r] = aq[k][e];
      }
  }
}

// grid (R, B): d_qt[b, r, :] = the slices' partials in slice order
__global__ __launch_bounds__(256) void crb_combine_kernel(const float* __restrict__ part, float* __restrict__ d_qt, int R,
                                                          int Dk, int slices) {
  const int q = blockIdx.x, b = blockIdx.y;
  for (int d = threadIdx.x; d < Dk; d += 256) {
    float t = 0.f;
    for (int s = 0; s < slices; ++s) t += part[(((long)b * slices + s) * R + q) * Dk + d];
    d_qt[((long)b * R + q) * Dk + d] = t;
  }
}

// ------------------------------------------------------------------------------------------------ host side
int cross_rows_backward_slices(int Lk) {
  const int per = crb_per(Lk);
  return (Lk + per - 1) / per;
}
// partial d_qt [B, slots, R, Dk] | SG [B, Lk, 32] | statistics [B, 16, 4]; slots = min(CRB_MAX_SLICES, ceil(Lk / 64))
// bounds the slice count and does not decrease with Lk (the slice count itself drops when `per` doubles)
static size_t crb_part_floats(int B, int R, int Lk, int Dk) {
  const size_t slots = (size_t)((Lk + 63) / 64 < CRB_MAX_SLICES ? (Lk + 63) / 64 : CRB_MAX_SLICES);
  return ((size_t)B * slots * R * Dk + 63) & ~(size_t)63;
}
size_t cross_rows_backward_ws_bytes(int B, int R, int Lk, int Dk) {
  if (B <= 0 || R <= 0 || Lk <= 0 || Dk <= 0) return 0;
  return (crb_part_floats(B, R, Lk, Dk) + (size_t)B * Lk * 32 + (size_t)B * 16 * 4) * 4;
}

template <typename T>
static void crb_t(const float* qt, const T* x, const float* dout, float* d_qt, float* d_x, int act, int accumulate, int B,
                  int R, int Lk, int Dk, float* ws, hipStream_t s) {
  const int per = crb_per(Lk), slices = cross_rows_backward_slices(Lk);
  float* part = ws;
  float* sg = part + crb_part_floats(B, R, Lk, Dk);
  float* stats = sg + (size_t)B * Lk * 32;
  float* pp = d_qt ? part : nullptr;
  const float neg = act == AACLIP_ACT_LEAKY ? 0.01f : (act == AACLIP_ACT_RELU ? 0.f : 1.0f);
  const int a = act != AACLIP_ACT_NONE;
  const dim3 g(slices, B), blk(256);
#define CRB(N)                                                                                                         \
  hipLaunchKernelGGL((crb_scores_kernel<T, N>), g, blk, 0, s, qt, dout, x, sg, R, Lk, per);                            \
  hipLaunchKernelGGL(crb_stats_kernel, dim3(R, B), blk, 0, s, sg, stats, Lk);                                          \
  hipLaunchKernelGGL((crb_grad_kernel<T, N>), g, blk, 0, s, qt, dout, x, sg, stats, d_x, pp, R, Lk, per, a, neg, accumulate)
  switch (Dk / 256) {
    case 1: CRB(1); break;
    case 2: CRB(2); break;
    case 3: CRB(3); break;
    case 4: CRB(4); break;
  }
#undef CRB
  if (d_qt) hipLaunchKernelGGL(crb_combine_kernel, dim3(R, B), blk, 0, s, part, d_qt, R, Dk, slices);
}

void launch_cross_rows_backward(int x_dtype, const float* qt, const void* x, const float* dout, float* d_qt, float* d_x,
                                int act, int accumulate, int B, int R, int Lk, int Dk, void* ws, hipStream_t s) {
  if (x_dtype == AACLIP_F32) crb_t<float>(qt, (const float*)x, dout, d_qt, d_x, act, accumulate, B, R, Lk, Dk, (float*)ws, s);
  else if (x_dtype == AACLIP_F16) crb_t<f16>(qt, (const f16*)x, dout, d_qt, d_x, act, accumulate, B, R, Lk, Dk, (float*)ws, s);
  else crb_t<bf16>(qt, (const bf16*)x, dout, d_qt, d_x, act, accumulate, B, R, Lk, Dk, (float*)ws, s);
}

}  // namespace aaclip
